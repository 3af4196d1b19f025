"""Behaviour cloning, the parts that need no GPU: the self-checks of the restatement (tests/bc_ref.py), the table of demonstration rows on a synthetic dataset
(bc_ref's builder by hand-written expectations, the package's against bc_ref's), every refusal of HipVecEnv.demonstrations / attach_bc by its message (an
env over CPU tensors and stand-in buffers and learners: nothing here opens the library), the new entry points in the header-derived prototypes, and the
tools' parsers.  The device side: tests/test_bc_gpu.py."""
import importlib.util
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import bc_ref as R
import replay_ref
import human_robot_gym_amd as hrg
from human_robot_gym_amd import _cstruct, _lib, bc, mixed, ppo, replay, rollout, sac
from human_robot_gym_amd._cstruct import CONST
from human_robot_gym_amd.dataset import STATE_BYTES, ExpertDataset
from human_robot_gym_amd.dist import packed_layout, packed_views
from human_robot_gym_amd.vec_env import _TorchBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4
SHAPES = [("sac", False), ("ppo", False), ("ppo", True)]


# ---- the restatement
@pytest.mark.parametrize("kind, separate", SHAPES)
def test_restatement_is_zero_at_its_own_outputs(kind, separate):
    K, A, depth = 6, 4, 2
    p = R.make_params(kind, K, A, depth, separate, seed=1)
    obs, _ = R.make_table(K, A, 32, seed=1)
    st = R.RefState(p, kind, depth, separate, torch.float64)
    own = R.prediction(st.p, torch.as_tensor(obs).double(), kind, depth, separate)
    out = st.step(obs, own, 1e-3)
    assert out["loss"] == 0.0
    assert all(bool((g == 0).all()) for g in out["grad"].values())
    assert all(torch.equal(st.p[k], torch.as_tensor(p[k]).double()) for k in p)   # Adam on a zero gradient moves nothing


@pytest.mark.parametrize("kind, separate", SHAPES)
def test_restatement_reaches_the_trunk_and_the_mean_head_only(kind, separate):
    K, A, depth = 6, 4, 3
    p = R.make_params(kind, K, A, depth, separate, seed=2)
    obs, act = R.make_table(K, A, 64, seed=2)
    st = R.RefState(p, kind, depth, separate, torch.float64)
    before = st.loss(obs, act)
    out = st.step(obs, act, 1e-3)
    if kind == "sac":
        reach = lambda k: k.startswith("actor.latent_pi.") or k.startswith("actor.mu.")   # noqa: E731
    else:
        trunk = "mlp_extractor.policy_net." if separate else "mlp_extractor.shared_net."
        reach = lambda k: k.startswith(trunk) or k.startswith("action_net.")   # noqa: E731
    assert sorted(out["reached"]) == sorted(k for k in p if reach(k))
    for k, g in out["grad"].items():
        if reach(k):
            assert float(g.abs().max()) > 0, k
            assert not torch.equal(st.p[k], torch.as_tensor(p[k]).double()), k
        else:   # SAC: actor.log_std.*, the critics, the targets, log_ent_coef; PPO: value_net.*, mlp_extractor.value_net.*, log_std
            assert bool((g == 0).all()) and torch.equal(st.p[k], torch.as_tensor(p[k]).double()), k
    unreached = [k for k in p if not reach(k)]
    assert ("actor.log_std.weight" in unreached) if kind == "sac" else ({"value_net.weight", "log_std"} <= set(unreached))
    if separate:
        assert "mlp_extractor.value_net.0.weight" in unreached
    assert out["loss"] == pytest.approx(before, rel=1e-12) and st.loss(obs, act) < before
    if kind == "sac":   # the dead units' rows are exact zeros
        assert bool((out["grad"]["actor.latent_pi.0.weight"][[3, 17]] == 0).all())


def test_restatement_loss_by_hand():
    """mean((tanh(mu) - a)^2) and mean((mu - a)^2) over rows and components, for a depth-1 actor written out."""
    K, A = 3, 2
    obs, act = R.make_table(K, A, 5, seed=3)
    o, a = torch.as_tensor(obs).double(), torch.as_tensor(act).double()
    p = R.make_params("sac", K, A, 1, False, seed=3)
    mu = torch.relu(o @ p["actor.latent_pi.0.weight"].T + p["actor.latent_pi.0.bias"]) @ p["actor.mu.weight"].T + p["actor.mu.bias"]
    assert R.RefState(p, "sac", 1).loss(obs, act) == pytest.approx(float(((torch.tanh(mu) - a) ** 2).sum() / (5 * A)), rel=1e-14)
    p = R.make_params("ppo", K, A, 1, False, seed=3)
    mu = torch.tanh(o @ p["mlp_extractor.shared_net.0.weight"].T + p["mlp_extractor.shared_net.0.bias"]) @ p["action_net.weight"].T + p["action_net.bias"]
    assert R.RefState(p, "ppo", 1).loss(obs, act) == pytest.approx(float(((mu - a) ** 2).sum() / (5 * A)), rel=1e-14)


# ---- the table
def _dataset(env_id="ReachHuman", cartesian=False):
    """Three episodes of 1, 2 and 5 transitions: obs row i holds i in every column (+ column / 100), the actions reach past the bounds."""
    lengths = [1, 2, 5]
    T, n = sum(lengths), len(lengths)
    obs = (np.arange(T + n, dtype=np.float32)[:, None] + np.arange(64, dtype=np.float32)[None, :] / 100).astype(np.float32)
    actions = np.linspace(-1.5, 1.5, T * 7).reshape(T, 7)
    return ExpertDataset(env_id, np.concatenate([[0], np.cumsum(lengths)]), np.zeros((T, STATE_BYTES), np.uint8), obs, actions, cartesian=cartesian, version="test")


def test_table_rows_and_time():
    ds = _dataset()
    rows, time = R.table_rows(ds.ep_offset)
    assert rows.tolist() == [0, 2, 3, 5, 6, 7, 8, 9]   # rows 1, 4 and 10 are the terminal ones
    assert time.dtype == np.float32 and time.tolist() == [0.0, 0.0, 0.5] + [np.float32(t / 5) for t in range(5)]
    got_rows, got_time = bc.demonstration_rows(ds)
    assert got_rows.tolist() == rows.tolist() and got_time.dtype == np.float32 and got_time.tobytes() == time.tobytes()


def test_table_observations_and_actions():
    ds = _dataset()
    cols, low, high = [2, 0, 5], np.array([-0.15] * 3 + [-1.0], np.float32), np.array([0.15] * 3 + [1.0], np.float32)
    mean, std = np.array([1.0, 2.0, 3.0, 0.5]), np.array([2.0, 0.5, 4.0, 0.25])
    rows, time = R.table_rows(ds.ep_offset)
    obs, act = R.table(ds.ep_offset, ds.obs, ds.actions, cols, low, high, "sac", observe_time=True, mean=mean, std=std)
    assert obs.shape == (8, 4) and obs.dtype == np.float32 and act.shape == (8, 4) and act.dtype == np.float32
    plain = np.concatenate([ds.obs[rows][:, cols], time[:, None]], axis=1)
    np.testing.assert_array_equal(obs, ((plain.astype(np.float64) - mean) / std).astype(np.float32))
    assert float(np.abs(ds.actions[:, :4]).max()) > 1.0   # (the inputs leave the bounds)
    lo, hi = low.astype(np.float64), high.astype(np.float64)
    clipped = np.clip(ds.actions[:, :4], lo, hi)
    assert act.min() == -1.0 and act.max() == 1.0
    np.testing.assert_array_equal(act, (2.0 * ((clipped - lo) / (hi - lo)) - 1.0).astype(np.float32))
    obs_p, act_p = R.table(ds.ep_offset, ds.obs, ds.actions, cols, low, high, "ppo")
    np.testing.assert_array_equal(obs_p, ds.obs[rows][:, cols])   # no time column, no statistics: a plain selection
    np.testing.assert_array_equal(act_p, clipped.astype(np.float32))   # the env's scale
    assert float(np.abs(act_p[:, :3]).max()) == np.float32(lo[0] * -1)
    for scale, want in ((True, act), (False, act_p)):
        np.testing.assert_array_equal(bc.demonstration_actions(ds, low, high, scale), want)
    joint = bc.demonstration_actions(ds, -np.ones(7, np.float32), np.ones(7, np.float32), True)
    np.testing.assert_array_equal(joint, np.clip(ds.actions, -1.0, 1.0).astype(np.float32))


def test_draws(oracle_lib):
    u01 = oracle_lib.hrgo_test_u01
    a, b = R.draw(u01, 7, 0, 96, 37), R.draw(u01, 7, 0, 32, 37)
    assert a.min() >= 0 and a.max() < 37 and len(set(a.tolist())) > 10
    assert a[:32].tolist() == b.tolist()   # a row's draw does not depend on the batch
    assert a.tolist() != R.draw(u01, 7, 1, 96, 37).tolist() and a.tolist() != R.draw(u01, 8, 0, 96, 37).tolist()
    assert R.draw(u01, 7, 3, 64, 1).tolist() == [0] * 64
    assert a[5] == int(np.floor(u01(7, 0, 5, 15, 0) * 37))   # STREAM_BC = 15, the next id after STREAM_PPO_ACT = 14


# ---- the refusals, on an env over CPU tensors
class _Batch:
    """What the device path reads of a HipBatch, as CPU tensors."""

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
    """Stands in for replay.ReplayBuffer / rollout.RolloutBuffer: the descriptor's sizes, and the view restated by replay_ref.view."""

    def __init__(self, desc, device=0, info_keys=None):
        self.desc, self.device = desc, torch.device("cpu")
        self.observe_time = bool(getattr(desc, "observe_time", 0))
        self.n, self.act_dim, self.obs_dim, self.n_steps = int(desc.n_envs), int(desc.act_dim), int(desc.n_obs_cols) + int(self.observe_time), int(getattr(desc, "n_steps", 0))

    def view(self, rows, time=None, out=None):
        d, K = self.desc, self.obs_dim
        norm = bool(getattr(d, "normalize", 0))
        return torch.from_numpy(replay_ref.view(rows.numpy(), list(d.obs_cols)[:int(d.n_obs_cols)], None if time is None else time.numpy(),
                                                list(d.mean)[:K] if norm else None, list(d.std)[:K] if norm else None))

    def observe(self, *a, **k):
        pass

    close = observe


def _learner(prefix, n_members=1):
    class Learner:
        _prefix = prefix

        def __init__(self, obs_dim, act_dim, *a, device=None, **kw):
            self.obs_dim, self.act_dim, self.n_members, self.device = int(obs_dim), int(act_dim), n_members, torch.device("cpu")

        def close(self):
            pass
    return Learner


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
    for mod, name, prefix, members in ((sac, "SacLearner", "hrg_sac", 1), (sac, "SacPopulation", "hrg_sac", 2), (ppo, "PpoLearner", "hrg_ppo", 1), (ppo, "PpoPopulation", "hrg_ppo", 2)):
        monkeypatch.setattr(mod, name, _learner(prefix, members))
    clips = hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300)
    return lambda **kw: hrg.HipVecEnv(N, env_kwargs=dict(horizon=5, shield_type="OFF", seed=3), clips=clips, backend=Backend, **kw)


def test_demonstrations_through_the_attached_view(make_env):
    """env.demonstrations hands the dataset's rows to the attached buffer's view and scales the actions by the learner's kind: bc_ref's table."""
    ds = _dataset()
    keys = ["robot0_joint_pos", "robot0_joint_vel"]
    rng = np.random.RandomState(0)
    env = make_env(obs_keys=keys, obs_norm=dict(mean=rng.uniform(-0.5, 0.5, 12), std=rng.uniform(0.5, 2.0, 12)))
    env.attach_replay(64)
    mean, std, _ = env._norm
    table = env.demonstrations(ds)
    want_obs, want_act = R.table(ds.ep_offset, ds.obs, ds.actions, env._cols, env.action_space.low, env.action_space.high, "sac", mean=mean, std=std)
    assert (table.kind, table.n_rows, table.obs_dim, table.act_dim) == ("sac", 8, 12, 7)
    assert table.observations.dtype == table.actions.dtype == torch.float32
    np.testing.assert_array_equal(table.observations.numpy(), want_obs)
    np.testing.assert_array_equal(table.actions.numpy(), want_act)
    env.close()
    env = make_env(obs_keys=keys)
    env.attach_rollout(4)
    table = env.demonstrations(ds)
    want_obs, want_act = R.table(ds.ep_offset, ds.obs, ds.actions, env._cols, env.action_space.low, env.action_space.high, "ppo")
    assert table.kind == "ppo"
    np.testing.assert_array_equal(table.observations.numpy(), want_obs)
    np.testing.assert_array_equal(table.actions.numpy(), want_act)
    env.attach_replay(64)
    with pytest.raises(ValueError, match="a replay and a rollout buffer are attached"):
        env.demonstrations(ds)
    assert env.demonstrations(ds, algorithm="sac").kind == "sac" and env.demonstrations(ds, algorithm="ppo").kind == "ppo"
    env.close()


def test_demonstrations_refusals(make_env):
    ds = _dataset()
    env = make_env()
    with pytest.raises(NotImplementedError, match=r"demonstrations: call attach_replay\(buffer_size\) \(SAC\) or attach_rollout\(n_steps\) \(PPO\) first"):
        env.demonstrations(ds)
    env.attach_replay(64)
    with pytest.raises(ValueError, match="demonstrations: a dataset of PickPlaceHumanCart, the env steps ReachHuman"):
        env.demonstrations(_dataset("PickPlaceHumanCart"))
    with pytest.raises(ValueError, match=r"demonstrations: the dataset's actions are Cartesian .*cartesian = True.*the env's are not"):
        env.demonstrations(_dataset(cartesian=True))
    hull = _dataset()
    hull.robot_geometry = "hull"
    with pytest.raises(ValueError, match="demonstrations: the dataset was recorded with robot_geometry = 'hull', the env collides the arm as 'capsule'"):
        env.demonstrations(hull)
    with pytest.raises(ValueError, match="algorithm = 'td3'"):
        env.demonstrations(ds, algorithm="td3")
    with pytest.raises(NotImplementedError, match="demonstrations: call attach_rollout first"):
        env.demonstrations(ds, algorithm="ppo")
    env.close()
    env = make_env(ik_position_delta=dict(action_limit=0.15))
    env.attach_replay(64)
    with pytest.raises(ValueError, match=r"demonstrations: the dataset's actions are joint space .*the env's are \(ik_position_delta\)"):
        env.demonstrations(ds)
    assert env.demonstrations(_dataset(cartesian=True)).act_dim == 4
    env.close()
    env = make_env(goal_env=True)
    with pytest.raises(NotImplementedError, match="demonstrations: goal_env: the hindsight feature row is another layout"):
        env.demonstrations(ds)
    env.close()
    stub = NS(slices=[slice(0, 2), slice(2, 4)], env_ids=["ReachHuman", "PickPlaceHumanCart"], step_async=None, close=lambda: None)
    with pytest.raises(NotImplementedError, match="demonstrations: a demonstration dataset is per task; use one HipVecEnv per task"):
        mixed.MixedHipVecEnv(stub).demonstrations(ds)


def test_attach_bc_refusals(make_env):
    ds = _dataset()
    env = make_env()
    env.attach_replay(64)
    table = env.demonstrations(ds)
    with pytest.raises(ValueError, match="attach_bc: dict is no table of demonstrations"):
        env.attach_bc({})
    with pytest.raises(NotImplementedError, match="attach_bc: call attach_sac first"):
        env.attach_bc(table)
    env.attach_sac_population(2)
    with pytest.raises(NotImplementedError, match="attach_bc: env.sac_population: behaviour cloning covers lone learners, not a population"):
        env.attach_bc(table)
    learner = env.attach_sac()
    for batch_size in (0, 40, 288):
        with pytest.raises(NotImplementedError, match=f"batch_size = {batch_size}: the kernels cover multiples of 32 from 32 to 256"):
            env.attach_bc(table, batch_size=batch_size)
    env.attach_rollout(4)
    with pytest.raises(ValueError, match="a table of kind 'ppo' for a sac learner"):
        bc.BehaviourCloning(learner, env.demonstrations(ds, algorithm="ppo"))
    narrow = bc.DemoTable(table.observations[:, :5], table.actions, "sac")
    with pytest.raises(ValueError, match="the table holds observations of 5 and actions of 7 values, the learner takes 18 and 7"):
        env.attach_bc(narrow)
    with pytest.raises(NotImplementedError, match="a population of 2 members; behaviour cloning covers lone learners"):
        bc.BehaviourCloning(env.sac_population, table)
    with pytest.raises(NotImplementedError, match="the kernels cover the actors of sac.SacLearner and ppo.PpoLearner"):
        bc.BehaviourCloning(NS(), table)
    with pytest.raises(ValueError, match="are not the rows of one table"):
        bc.DemoTable(table.observations[:3], table.actions, "sac")
    assert env.bc is None
    env.close()


# ---- the ABI and the tools
def test_prototypes_come_from_the_header():
    names = ["hrg_bc_create_sac", "hrg_bc_create_ppo", "hrg_bc_destroy", "hrg_bc_sizes", "hrg_bc_step", "hrg_bc_export"]
    assert all(n in _cstruct.PROTOTYPES and n in _lib.EXPORTS for n in names)
    import ctypes
    vp = ctypes.c_void_p
    assert _cstruct.PROTOTYPES["hrg_bc_step"] == (ctypes.c_int, [vp, vp, vp, ctypes.c_int64, vp, vp, vp, vp, ctypes.c_double, vp])
    assert _cstruct.PROTOTYPES["hrg_bc_create_sac"] == (ctypes.c_int, [vp, vp, ctypes.c_int32, vp])
    assert _cstruct.PROTOTYPES["hrg_bc_destroy"][0] is None
    assert [n for n, _ in _cstruct.BcDesc._fields_] == ["kind", "batch_size", "seed"] and ctypes.sizeof(_cstruct.BcDesc) == 16
    assert (CONST["HRG_BC_MAX_BATCH"], CONST["HRG_BC_SAC"], CONST["HRG_BC_PPO"]) == (256, 0, 1)


def _tool(name):
    spec = importlib.util.spec_from_file_location("tool_" + name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_parsers():
    a = _tool("pretrain_bc").ap.parse_args(["--env", "ReachHuman", "--dataset", "reach-demo", "--out", "models/bc/model_final.npz"])
    assert (a.algorithm, a.steps, a.batch_size, a.learning_rate, a.seed, a.eval_episodes) == ("sac", 1000, 128, 1e-3, 0, 0)
    a = _tool("pretrain_bc").ap.parse_args(["--env", "ReachHuman", "--dataset", "d", "--out", "o.npz", "--algorithm", "ppo", "--steps", "5", "--eval-episodes", "3"])
    assert (a.algorithm, a.steps, a.eval_episodes) == ("ppo", 5, 3)
    with pytest.raises(SystemExit):
        _tool("pretrain_bc").ap.parse_args(["--env", "ReachHuman", "--dataset", "d", "--out", "o.npz", "--algorithm", "td3"])
    for name, extra in (("train_sac", ["--gradient-steps", "1"]), ("train_ppo", [])):
        ap = _tool(name).ap
        assert ap.parse_args(extra).init_checkpoint is None
        assert ap.parse_args(extra + ["--init-checkpoint", "models/bc/model_final.npz"]).init_checkpoint == "models/bc/model_final.npz"
