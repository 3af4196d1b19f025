"""Adversarial imitation, the parts that need no GPU: the self-checks of the restatement (tests/disc_ref.py: the gradient by finite differences, the reward
against its textbook forms, the separable fixture's margin), the descriptor from its keywords, every Python-side refusal by its message (tables of CPU tensors,
an env over CPU tensors and stand-in buffers and learners: nothing here opens the library), the new entry points in the header-derived prototypes, and the
tools' parsers.  The device side: tests/test_adversarial_gpu.py."""
import ctypes
import importlib.util
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import disc_ref as R
import replay_ref
import human_robot_gym_amd as hrg
from human_robot_gym_amd import _cstruct, _lib, adversarial, bc, mixed, ppo, replay, rollout, sac
from human_robot_gym_amd._cstruct import CONST
from human_robot_gym_amd._learner import LearnerParams
from human_robot_gym_amd.dataset import STATE_BYTES, ExpertDataset
from human_robot_gym_amd.dist import packed_layout, packed_views
from human_robot_gym_amd.vec_env import _TorchBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4


# ---- the restatement
def test_restatement_gradient_by_finite_differences():
    """K = 1, A = 1, depth 1, B = 32: every entry of the autograd gradient against central differences of the loss written out by hand."""
    K = A = depth = 1
    B = 32
    p = R.make_params(K, A, depth, seed=4)
    eo, ea = R.make_rows(K, A, B, seed=1)
    po, pa = R.make_rows(K, A, B, seed=2)
    out = R.RefState(p, depth, "tanh", torch.float64).step(eo, ea, po, pa, 1e-3)

    def loss(q):
        def d(o, a):
            x = np.concatenate([o, a], axis=1).astype(np.float64)
            return (np.tanh(x @ q["disc.0.weight"].T + q["disc.0.bias"]) @ q["disc.2.weight"].T + q["disc.2.bias"])[:, 0]
        softplus = lambda x: np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))   # noqa: E731
        return (softplus(-d(eo, ea)).sum() + softplus(d(po, pa)).sum()) / (2 * B)

    q = {k: v.numpy().copy() for k, v in p.items()}
    assert out["loss"] == pytest.approx(loss(q), rel=1e-13)
    h, worst = 1e-6, 0.0
    for k in q:
        flat = q[k].reshape(-1)   # (a view)
        for i in range(flat.size):
            keep = flat[i]
            flat[i] = keep + h
            up = loss(q)
            flat[i] = keep - h
            down = loss(q)
            flat[i] = keep
            worst = max(worst, abs((up - down) / (2 * h) - float(out["grad"][k].reshape(-1)[i])))
    assert sum(v.size for v in q.values()) == 64 * 2 + 64 + 64 + 1 and worst < 1e-8, worst
    assert out["logits"].shape == (2 * B,) and 0.0 <= out["expert_accuracy"] <= 1.0 and 0.0 <= out["policy_accuracy"] <= 1.0


def test_restatement_adam_moves_every_entry_and_counts():
    K, A, depth, B = 6, 4, 2, 32
    p = R.make_params(K, A, depth, seed=2)
    st = R.RefState(p, depth, "relu", torch.float64)
    out = st.step(*R.make_rows(K, A, B, seed=1), *R.make_rows(K, A, B, seed=2), 1e-3)
    assert st.steps == 1 and sorted(out["grad"]) == sorted(p)
    for k in ("disc.0.weight", "disc.2.weight", "disc.4.weight", "disc.4.bias"):
        assert float(out["grad"][k].abs().max()) > 0 and not torch.equal(st.p[k], p[k])
    d = out["logits"]
    assert out["expert_accuracy"] == float((d[:B] > 0).sum()) / B and out["policy_accuracy"] == float((d[B:] < 0).sum()) / B


def test_restatement_reward_forms():
    """softplus(d) = -log(1 - sigmoid(d)) and d = log(sigmoid(d) / (1 - sigmoid(d))) at moderate d; the mix with the env's reward."""
    K, A, depth = 6, 4, 2
    p = R.make_params(K, A, depth, seed=3)
    p["disc.4.weight"] *= 8.0   # logits of a few units
    obs, act = R.make_rows(K, A, 50, seed=3)
    gail, d = R.reward(p, obs, act, depth, kind="gail")
    airl, d2 = R.reward(p, obs, act, depth, kind="airl")
    D = torch.sigmoid(d)
    assert torch.equal(d, d2) and 0.5 < float(d.abs().max()) < 20.0
    np.testing.assert_allclose(gail.numpy(), -torch.log(1.0 - D).numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(airl.numpy(), torch.log(D / (1.0 - D)).numpy(), rtol=1e-12, atol=1e-13)
    r_env = torch.linspace(-2.0, 2.0, 50, dtype=torch.float64)
    mix, _ = R.reward(p, obs, act, depth, env_rewards=r_env.reshape(-1, 1), alpha=0.25, kind="gail")
    np.testing.assert_allclose(mix.numpy(), (0.25 * gail + 0.75 * r_env).numpy(), rtol=1e-15)
    assert torch.equal(R.reward(p, obs, act, depth, env_rewards=r_env, alpha=0.0)[0], r_env) and torch.equal(R.reward(p, obs, act, depth, env_rewards=r_env, alpha=1.0)[0], gail)


def test_separable_fixture_keeps_its_margin():
    """On the fixture of the accuracy test |d| > 0.1 on every row in ref64, before and after the update, and neither accuracy is 0 or 1: a count the device
    gets wrong by one row shows, and no row sits where float32 rounding could move it across d = 0."""
    p, tobs, tact, idx, pobs, pact = R.separable_case()
    c = R.SEPARABLE
    assert tobs.shape == (c["n_rows"], c["obs_dim"]) and pact.shape == (c["batch"], c["act_dim"]) and idx.shape == (c["batch"],) and idx.max() < c["n_rows"]
    st = R.RefState(p, 1, "relu", torch.float64)
    out = st.step(tobs[idx], tact[idx], pobs, pact, 1e-3)
    assert float(out["logits"].abs().min()) > 0.1
    assert float(torch.cat([st.logits(tobs[idx], tact[idx]), st.logits(pobs, pact)]).abs().min()) > 0.1
    assert 0.5 < out["expert_accuracy"] < 1.0 and 0.5 < out["policy_accuracy"] < 1.0
    o32 = R.RefState(p, 1, "relu", torch.float32).step(tobs[idx], tact[idx], pobs, pact, 1e-3)
    assert (o32["expert_accuracy"], o32["policy_accuracy"]) == (out["expert_accuracy"], out["policy_accuracy"])


def test_draws(oracle_lib):
    u01 = oracle_lib.hrgo_test_u01
    a, b = R.draw(u01, 7, 0, 96, 37), R.draw(u01, 7, 0, 32, 37)
    assert a.min() >= 0 and a.max() < 37 and len(set(a.tolist())) > 10
    assert a[:32].tolist() == b.tolist()   # a row's draw does not depend on the batch
    assert a.tolist() != R.draw(u01, 7, 1, 96, 37).tolist() and a.tolist() != R.draw(u01, 8, 0, 96, 37).tolist()
    assert R.draw(u01, 7, 3, 64, 1).tolist() == [0] * 64
    assert a[5] == int(np.floor(u01(7, 0, 5, 17, 0) * 37))   # STREAM_DISC = 17, the next id after STREAM_DAGGER = 16


# ---- the package's side without a GPU
def test_parameters_move_between_the_restatement_and_the_package():
    """disc_ref.make_params is the initialisation of the Python class (LearnerParams over adversarial.param_layout), entry for entry."""
    for K, A, depth in ((1, 1, 1), (18, 4, 3), (64, 7, 2)):
        layout, n = adversarial.param_layout(K, A, depth)
        assert n == 64 * (K + A) + 64 + (depth - 1) * (64 * 64 + 64) + 64 + 1
        own = LearnerParams(layout, n, 9, "cpu").state_dict()
        ref = R.make_params(K, A, depth, seed=9)
        assert list(own) == list(ref) and all(torch.equal(own[k].double(), ref[k]) for k in ref)
        assert layout[f"disc.{2 * depth}.weight"][1] == (1, 64) and layout["disc.0.weight"] == (0, (64, K + A))


def test_descriptor_from_its_keywords():
    d = adversarial.build_disc_desc(18, 4)
    assert (d.obs_dim, d.act_dim, d.depth, d.hidden, d.batch_size, d.activation, d.reward_kind, d.seed) == (18, 4, 2, 64, 128, CONST["HRG_DISC_RELU"], CONST["HRG_DISC_REWARD_GAIL"], 0)
    d = adversarial.build_disc_desc(64, 7, net_arch=[64] * 3, activation="tanh", batch_size=256, reward="airl", seed=-1)
    assert (d.obs_dim, d.act_dim, d.depth, d.batch_size, d.activation, d.reward_kind, d.seed) == (64, 7, 3, 256, CONST["HRG_DISC_TANH"], CONST["HRG_DISC_REWARD_AIRL"], 2 ** 64 - 1)
    assert (CONST["HRG_DISC_MAX_BATCH"], CONST["HRG_DISC_REWARD_GAIL"], CONST["HRG_DISC_REWARD_AIRL"]) == (256, 0, 1)


def _table(K=6, A=4, n=5, kind="sac"):
    return bc.DemoTable(torch.zeros(n, K), torch.zeros(n, A), kind)


def test_constructor_refusals_come_before_the_library():
    """Each is raised before `_open`, which on a machine without a GPU would raise RuntimeError and with one would allocate."""
    D = adversarial.Discriminator
    with pytest.raises(ValueError, match="a table of kind 'ppo'.*policy's scale.*build the table with the replay buffer attached"):
        D(_table(kind="ppo"))
    with pytest.raises(ValueError, match="dict is no table of demonstrations"):
        D({})
    for arch in ([], [64] * 4, [32, 32], [64, 128]):
        with pytest.raises(NotImplementedError, match=r"net_arch = .*hidden width 64 and depth 1 \.\. 3"):
            D(_table(), net_arch=arch)
    for batch_size in (0, 40, 288):
        with pytest.raises(NotImplementedError, match=f"batch_size = {batch_size}: the kernels cover multiples of 32 from 32 to 256"):
            D(_table(), batch_size=batch_size)
    with pytest.raises(NotImplementedError, match="obs_dim = 65"):
        D(_table(K=65))
    with pytest.raises(NotImplementedError, match="act_dim = 8"):
        D(_table(A=8))
    with pytest.raises(ValueError, match="activation = 'gelu': one of"):
        D(_table(), activation="gelu")
    with pytest.raises(ValueError, match="reward = 'wgan': one of"):
        D(_table(), reward="wgan")
    for lr in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="learning_rate = .*a finite learning rate that is not negative"):
            D(_table(), learning_rate=lr)
    for alpha in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="alpha = .* outside"):
            adversarial.check_alpha(alpha)
    assert adversarial.check_alpha(0) == 0.0 and adversarial.check_alpha(1) == 1.0


def test_train_sac_refusals():
    disc = NS(batch_size=128, obs_dim=18, act_dim=4)
    buf = NS(obs_dim=18, act_dim=4)
    with pytest.raises(ValueError, match="the discriminator's batch_size = 128, the learner's = 64"):
        adversarial.train_sac(NS(batch_size=64, obs_dim=18, act_dim=4, n_members=1), buf, disc, 1)
    with pytest.raises(ValueError, match="the discriminator takes observations of 18 and actions of 4 values, the learner 18 and 7"):
        adversarial.train_sac(NS(batch_size=128, obs_dim=18, act_dim=7, n_members=1), buf, disc, 1)
    with pytest.raises(NotImplementedError, match="a lone sac.SacLearner on a replay.ReplayBuffer"):
        adversarial.train_sac(NS(batch_size=128, obs_dim=18, act_dim=4, n_members=2), buf, disc, 1)
    with pytest.raises(NotImplementedError, match="a lone sac.SacLearner on a replay.ReplayBuffer"):
        adversarial.train_sac(NS(batch_size=128, obs_dim=18, act_dim=4, n_members=1), NS(sample_features=None), disc, 1)
    ok = NS(batch_size=128, obs_dim=18, act_dim=4, n_members=1, _check_buffer=lambda *a: None)
    with pytest.raises(ValueError, match="alpha = 2 outside"):
        adversarial.train_sac(ok, buf, disc, 1, alpha=2)
    adversarial.train_sac(ok, buf, disc, 0)   # no step: nothing is sampled


# ---- the refusals of attach_discriminator, on an env over CPU tensors (the stand-ins of tests/test_bc.py)
class _Batch:
    def __init__(self, n):
        self.n, self.device = n, torch.device("cpu")
        self.packed = torch.zeros(packed_layout(n)["total"], dtype=torch.uint8)
        for k, v in packed_views(self.packed, n).items():
            setattr(self, k, v)

    def reset(self):
        self.obs.zero_()

    def close(self):
        pass


class _Buffer:
    def __init__(self, desc, device=0, info_keys=None):
        self.desc, self.device = desc, torch.device("cpu")
        self.observe_time = bool(getattr(desc, "observe_time", 0))
        self.n, self.act_dim, self.obs_dim, self.n_steps = int(desc.n_envs), int(desc.act_dim), int(desc.n_obs_cols) + int(self.observe_time), int(getattr(desc, "n_steps", 0))

    def view(self, rows, time=None, out=None):
        d = self.desc
        return torch.from_numpy(replay_ref.view(rows.numpy(), list(d.obs_cols)[:int(d.n_obs_cols)], None if time is None else time.numpy(), None, None))

    def observe(self, *a, **k):
        pass

    close = observe


@pytest.fixture
def make_env(monkeypatch):
    class Backend(_TorchBackend):
        def __init__(self, desc, clips, n_envs, env_id0):
            self.torch, self.batch, self.n = torch, _Batch(n_envs), n_envs
            self._host = torch.zeros_like(self.batch.packed)
            v = packed_views(self._host.numpy(), n_envs)
            self.obs, self.term_obs, self.reward, self.info, self.done = v["obs"], v["term_obs"], v["reward"], v["info"], v["done"]
            self.imit = self.sir = self.path = None

    monkeypatch.setattr(replay, "ReplayBuffer", _Buffer)
    monkeypatch.setattr(rollout, "RolloutBuffer", _Buffer)
    clips = hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300)
    return lambda **kw: hrg.HipVecEnv(N, env_kwargs=dict(horizon=5, shield_type="OFF", seed=3), clips=clips, backend=Backend, **kw)


def _dataset(env_id="ReachHuman"):
    lengths = [1, 2, 5]
    T, n = sum(lengths), len(lengths)
    obs = (np.arange(T + n, dtype=np.float32)[:, None] + np.arange(64, dtype=np.float32)[None, :] / 100).astype(np.float32)
    return ExpertDataset(env_id, np.concatenate([[0], np.cumsum(lengths)]), np.zeros((T, STATE_BYTES), np.uint8), obs, np.linspace(-1.5, 1.5, T * 7).reshape(T, 7), version="test")


def test_attach_discriminator_refusals(make_env):
    ds = _dataset()
    env = make_env()
    assert env.discriminator is None
    with pytest.raises(NotImplementedError, match=r"demonstrations: call attach_replay\(buffer_size\) \(SAC\) or attach_rollout\(n_steps\) \(PPO\) first"):
        env.attach_discriminator(ds)   # a dataset goes through env.demonstrations, whose refusals apply unchanged
    env.attach_rollout(4)
    with pytest.raises(ValueError, match="discriminator: a table of kind 'ppo'"):
        env.attach_discriminator(ds)
    with pytest.raises(ValueError, match="discriminator: a table of kind 'ppo'"):
        env.attach_discriminator(env.demonstrations(ds))
    env.attach_replay(64)
    with pytest.raises(ValueError, match="demonstrations: a dataset of PickPlaceHumanCart, the env steps ReachHuman"):
        env.attach_discriminator(_dataset("PickPlaceHumanCart"))
    with pytest.raises(NotImplementedError, match="batch_size = 40: the kernels cover multiples of 32 from 32 to 256"):
        env.attach_discriminator(ds, batch_size=40)   # (with both buffers attached the replay buffer's view is taken)
    with pytest.raises(ValueError, match="reward = 'wgan'"):
        env.attach_discriminator(env.demonstrations(ds, algorithm="sac"), reward="wgan")
    assert env.discriminator is None
    env.close()
    env = make_env(goal_env=True)
    with pytest.raises(NotImplementedError, match="attach_discriminator: goal_env: the hindsight feature row is another layout \\(adversarial imitation covers flat observations\\)"):
        env.attach_discriminator(ds)
    env.close()
    stub = NS(slices=[slice(0, 2), slice(2, 4)], env_ids=["ReachHuman", "PickPlaceHumanCart"], step_async=None, close=lambda: None)
    with pytest.raises(NotImplementedError, match="attach_discriminator: a demonstration dataset is per task; use one HipVecEnv per task"):
        mixed.MixedHipVecEnv(stub).attach_discriminator(ds)
    assert "discriminator" in hrg.HipVecEnv.attach_discriminator.__doc__ and sac.SacLearner is not None and ppo.PpoLearner is not None


def test_another_backend_is_refused_by_name():
    from helpers import OracleBackend
    clips, ek = hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300), dict(shield_type="OFF", horizon=5)
    env = hrg.HipVecEnv(3, env_kwargs=ek, clips=clips, backend=OracleBackend(hrg.build_model_desc(ek, n_clips=2), clips, 3))
    with pytest.raises(NotImplementedError, match="attach_discriminator: the discriminator kernels run in the HIP library; another backend has none"):
        env.attach_discriminator(_dataset())
    env.close()


# ---- the ABI and the tools
def test_prototypes_come_from_the_header():
    names = ["hrg_disc_create", "hrg_disc_destroy", "hrg_disc_sizes", "hrg_disc_step", "hrg_disc_reward", "hrg_disc_export", "hrg_disc_restore"]
    assert all(n in _cstruct.PROTOTYPES and n in _lib.EXPORTS for n in names)
    vp = ctypes.c_void_p
    assert _cstruct.PROTOTYPES["hrg_disc_step"] == (ctypes.c_int, [vp, vp, vp, ctypes.c_int64, vp, vp, vp, vp, vp, vp, ctypes.c_double, vp])
    assert _cstruct.PROTOTYPES["hrg_disc_reward"] == (ctypes.c_int, [vp, vp, vp, vp, ctypes.c_int32, vp, ctypes.c_double, vp, vp, vp])
    assert _cstruct.PROTOTYPES["hrg_disc_create"] == (ctypes.c_int, [vp, ctypes.c_int32, vp])
    assert _cstruct.PROTOTYPES["hrg_disc_restore"] == (ctypes.c_int, [vp, ctypes.c_uint64]) and _cstruct.PROTOTYPES["hrg_disc_destroy"][0] is None
    fields = [n for n, _ in _cstruct.DiscDesc._fields_]
    assert fields == ["obs_dim", "act_dim", "depth", "hidden", "batch_size", "activation", "reward_kind", "reserved_", "seed"] and ctypes.sizeof(_cstruct.DiscDesc) == 40


def _tool(name):
    spec = importlib.util.spec_from_file_location("tool_" + name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_parsers():
    ap = _tool("train_sac_gail").ap
    a = ap.parse_args(["--dataset", "reach-demo", "--gradient-steps", "800"])
    assert (a.env_id, a.alpha, a.reward, a.disc_every, a.disc_lr, a.batch_size, a.model_dir, a.save_freq, a.eval_episodes) == ("ReachHuman", 1.0, "gail", 1, 3e-4, 128, None, 0, 0)
    a = ap.parse_args(["--dataset", "d", "--gradient-steps", "1", "--alpha", "0.25", "--reward", "airl", "--disc-every", "4", "--disc-lr", "1e-4", "--model-dir", "models/x"])
    assert (a.alpha, a.reward, a.disc_every, a.disc_lr, a.model_dir) == (0.25, "airl", 4, 1e-4, "models/x")
    for bad in (["--gradient-steps", "1"], ["--dataset", "d", "--gradient-steps", "1", "--reward", "wgan"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    b = _tool("bench_gail")
    a = b.ap.parse_args([])
    assert (a.blocks, a.steps, a.rows, a.out) == (7, 200, 100_000, "profiles/r33_disc.json") and (b.B, b.K, b.A, b.ARCH) == (128, 18, 4, [64, 64, 64])
