"""DAgger, the parts that need no GPU: the self-checks of the restatement (tests/dagger_ref.py: the key of the draws, the extremes of beta, the ring behind a
pinned prefix), label inputs on which a float32 slip shows, the new entry points in the header-derived prototypes, every refusal of attach_dagger /
collect_dagger / dagger.Dagger by its message, and the lifecycle of the path on a recording batch with CPU tensors, in the manner of tests/test_device_path.py
(whose FakeBatch, buffers and log are used as they are).  The device side: tests/test_dagger_gpu.py."""
import ctypes
import importlib.util
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import dagger_ref as R
import human_robot_gym_amd as hrg
from helpers import OracleBackend
from human_robot_gym_amd import _cstruct, _lib, bc, dagger, mixed, ppo, replay, rollout, sac
from human_robot_gym_amd._cstruct import CONST
from human_robot_gym_amd.dist import packed_views
from human_robot_gym_amd.vec_env import _TorchBackend
from test_device_path import FakeBatch, Log, N, fake_buffer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACT = CONST["HRG_ACT_DIM"]


# ---- the restatement
def test_draw_key_and_stream(oracle_lib):
    u01 = oracle_lib.hrgo_test_u01
    assert R.STREAM_DAGGER == 16   # the next id after STREAM_BC = 15
    header = open(os.path.join(ROOT, "human-robot-gym_amd", "csrc", "hrgym_dagger.h")).read()
    assert "enum { STREAM_DAGGER = 16 };" in header and "#pragma once" in header
    u = R.draws(u01, 7, 3, 6, env_id0=100)
    assert u[2] == u01(7, 3, 102, 16, 0)   # (seed, call, global env id, stream, 0)
    assert 0.0 <= u.min() and u.max() < 1.0 and len(set(u.tolist())) == 6
    assert R.draws(u01, 7, 3, 4, env_id0=102)[0] == u[2]   # a shard's env draws what the whole batch's env draws
    assert u.tolist() != R.draws(u01, 7, 4, 6, env_id0=100).tolist() and u.tolist() != R.draws(u01, 8, 3, 6, env_id0=100).tolist()   # per step, per seed


def _step_inputs(rng, n, K, A):
    return rng.uniform(-1, 1, (n, K)).astype(np.float32), rng.uniform(-1.2, 1.2, (n, A)).astype(np.float32), rng.uniform(-1.3, 1.3, (n, ACT))


@pytest.mark.parametrize("kind", ["sac", "ppo"])
def test_beta_extremes(oracle_lib, kind):
    u01 = oracle_lib.hrgo_test_u01
    n, K, A = 5, 3, 4
    x, low, high = R.label_inputs(n, A, 0.15, seed=1)
    rng = np.random.RandomState(2)
    view, learner, _ = _step_inputs(rng, n, K, A)
    learner[:, :3] *= 0.2
    never, always = (R.Dagger(kind, n, K, A, 2, low, high, seed=5) for _ in range(2))
    a, b = never.step(u01, view, learner, x, 0.0), always.step(u01, view, learner, x, 1.0)
    assert not a["expert"].any() and b["expert"].all()
    clipped = np.clip(x[:, :A], low, high)
    np.testing.assert_array_equal(b["rows"][:, :A], clipped)
    assert not b["rows"][:, A:].any() and not a["rows"][:, A:].any()
    if kind == "sac":
        np.testing.assert_array_equal(a["rows"][:, :A], low + 0.5 * (learner.astype(np.float64) + 1.0) * (high - low))
        np.testing.assert_array_equal(b["label"], bc.demonstration_actions(NS(actions=x), low, high, True))
        assert b["label"].min() == -1.0 and b["label"].max() == 1.0
    else:
        np.testing.assert_array_equal(a["rows"][:, :A], np.clip(learner, low.astype(np.float32), high.astype(np.float32)).astype(np.float64))
        np.testing.assert_array_equal(b["label"], clipped.astype(np.float32))
    np.testing.assert_array_equal(a["kept"], learner)   # the learner's own row
    np.testing.assert_array_equal(b["kept"], b["label"])   # the label
    np.testing.assert_array_equal(a["label"], b["label"])   # the label does not depend on who drives
    np.testing.assert_array_equal(never.stats[:, :2], [[1.0, 0.0]] * n)
    np.testing.assert_array_equal(always.stats[:, :2], [[1.0, 1.0]] * n)
    at = learner if kind == "sac" else np.clip(learner, low.astype(np.float32), high.astype(np.float32))
    np.testing.assert_allclose(never.stats[:, 2], ((at.astype(np.float64) - a["label"].astype(np.float64)) ** 2).sum(axis=1), rtol=1e-14)
    np.testing.assert_array_equal(never.stats[:, 2], always.stats[:, 2])   # the error is the learner's, whoever drives


def test_ring_wraps_behind_the_pinned_rows(oracle_lib):
    u01 = oracle_lib.hrgo_test_u01
    n, K, A, cap, P = 3, 2, 4, 3, 7
    rng = np.random.RandomState(3)
    pinned = rng.uniform(-1, 1, (P, K)).astype(np.float32), rng.uniform(-1, 1, (P, A)).astype(np.float32)
    _, low, high = R.label_inputs(1, A, 0.2, seed=0)
    d = R.Dagger("sac", n, K, A, cap, low, high, seed=1, pinned=pinned)
    assert d.n_rows == P and d.observations.shape == (P + cap * n, K)
    empty = R.Dagger("sac", n, K, A, cap, low, high, seed=1)
    assert empty.n_rows == 0
    views = []
    for t in range(5):
        view, learner, x = _step_inputs(rng, n, K, A)
        views.append(view)
        out = d.step(u01, view, learner, x, 0.4)
        assert out["slot"] == t % cap and d.slot == (t + 1) % cap and d.calls == t + 1
        assert d.n_rows == P + min(t + 1, cap) * n
        np.testing.assert_array_equal(d.observations[P + (t % cap) * n:P + (t % cap + 1) * n], view)   # slot s, env e: row pinned + s n + e
        np.testing.assert_array_equal(d.actions[d.slot_rows(out["slot"])], out["label"])
    np.testing.assert_array_equal(d.observations[:P], pinned[0])
    np.testing.assert_array_equal(d.actions[:P], pinned[1])
    for slot, t in ((0, 3), (1, 4), (2, 2)):   # steps 3 and 4 overwrote 0 and 1
        np.testing.assert_array_equal(d.observations[d.slot_rows(slot)], views[t])
    assert d.stats[:, 0].tolist() == [5.0] * n and 0 < d.stats[:, 1].sum() < 5 * n


# ---- label inputs on which a float32 slip shows
@pytest.mark.parametrize("limit", [0.1, 0.15, 0.2, 1.0])
def test_label_inputs_catch_a_float32_restatement(limit):
    n, A = 4096, 5
    x, low, high = R.label_inputs(n, A, limit, seed=int(limit * 100))
    ref = R.label(x, low, high, "sac")
    assert ref.dtype == np.float32 and ref.min() == -1.0 and ref.max() == 1.0
    np.testing.assert_array_equal(ref, bc.demonstration_actions(NS(actions=x), low, high, True))
    assert set(np.unique(ref[:, A - 1]).tolist()) == {-1.0, np.float32(2.0 * ((0.3 + 1.0) / 2.0) - 1.0), 1.0}   # the gripper column
    motions = np.s_[:, :A - 1]
    assert ref[motions].size == 16384
    inside = np.abs(x[motions]) < limit
    assert 0.7 < inside.mean() < 0.85   # 1 / 1.3 of the motions lie inside the bounds, the rest is clipped to exactly -1 or 1
    slip = R.label(x, low, high, "sac", dtype=np.float32)
    share = float((slip[motions] != ref[motions]).mean())
    print(f"limit {limit}: a float32 restatement differs in {100 * share:.1f} % of 16384 motion values")
    assert share > 0.05
    recip = R.label(x, low, high, "sac", reciprocal=True)
    differ = int((recip[motions] != ref[motions]).sum())
    print(f"limit {limit}: the float64 reciprocal-multiply variant differs in {differ} of 16384")
    assert differ == 0
    np.testing.assert_array_equal(R.label(x, low, high, "ppo"), np.clip(x[:, :A], low, high).astype(np.float32))


# ---- the ABI
def test_prototypes_come_from_the_header():
    names = ["hrg_dagger_create", "hrg_dagger_destroy", "hrg_dagger_step", "hrg_dagger_sizes", "hrg_dagger_stats"]
    assert all(n in _cstruct.PROTOTYPES and n in _lib.EXPORTS for n in names)
    vp, P = ctypes.c_void_p, _cstruct.PROTOTYPES
    assert P["hrg_dagger_create"] == (ctypes.c_int, [vp, ctypes.c_int32, vp])
    assert P["hrg_dagger_destroy"] == (None, [vp])
    assert P["hrg_dagger_step"] == (ctypes.c_int, [vp, vp, vp, vp, ctypes.c_double, vp, vp, vp, vp, vp])
    assert P["hrg_dagger_sizes"] == (ctypes.c_int, [vp, vp])
    assert P["hrg_dagger_stats"] == (ctypes.c_int, [vp, vp, ctypes.c_int32])
    assert [n for n, _ in _cstruct.DaggerDesc._fields_] == ["kind", "n_envs", "env_id0", "obs_dim", "act_dim", "capacity_steps", "pinned_rows", "seed", "act_low", "act_high"]
    assert ctypes.sizeof(_cstruct.DaggerDesc) == 40 + 2 * 8 * ACT
    assert (CONST["HRG_DAGGER_STATS_DIM"], CONST["HRG_DAGGER_STEPS"], CONST["HRG_DAGGER_EXPERT_STEPS"], CONST["HRG_DAGGER_SQ_ERROR"]) == (3, 0, 1, 2)
    base = open(os.path.join(ROOT, "human-robot-gym_amd", "csrc", "hrgym_hip.hip")).read()
    assert base.index('#include "hrgym_bc.h"') < base.index('#include "hrgym_dagger.h"') < base.index("#include \"hrgym_host.h\"")


# ---- the env over CPU tensors: a recording batch with an expert buffer, recording buffers, learners and dagger handle
class ExpertBatch(FakeBatch):
    def __init__(self, log):
        super().__init__(log)
        self._expert_act = torch.full((N, ACT), 0.25, dtype=torch.float64)

    def expert_actions(self):
        self.log.add("batch", "expert_actions")
        return self._expert_act


def fake_learner(slot, log, n_members=1):
    class FakeLearner:
        _prefix = "hrg_" + slot.split("_")[0]

        def __init__(self, obs_dim, act_dim, *a, device=None, **kw):
            self.obs_dim, self.act_dim, self.n_members, self.device = int(obs_dim), int(act_dim), n_members, torch.device("cpu")
            self.actions = torch.full((N, self.act_dim), 0.5, dtype=torch.float32)
            log.add(slot, "new")

        def act(self, obs, deterministic=False):
            log.add(slot, "act", obs, deterministic)
            return self.actions

        def policy(self, obs, deterministic=False):
            log.add(slot, "policy", obs, deterministic)
            return self.actions, torch.zeros(N), torch.zeros(N)

        def close(self):
            log.add(slot, "close")
    return FakeLearner


def fake_dagger(log, made):
    class FakeDagger:
        def __init__(self, kind, n_envs, obs_dim, act_dim, capacity_steps, low, high, beta=0.5, pinned=None, seed=0, env_id0=0, device=0):
            self.name = f"dagger{len(made)}"
            made.append(self)
            self.args = dict(kind=kind, n_envs=n_envs, obs_dim=obs_dim, act_dim=act_dim, capacity_steps=capacity_steps, low=low, high=high, pinned=pinned, seed=seed,
                             env_id0=env_id0)
            self.beta, self.n_calls, self.table = beta, 0, NS(kind=kind, obs_dim=obs_dim, act_dim=act_dim, n_rows=0, device=torch.device("cpu"))
            log.add(self.name, "new")

        def step(self, view, learner_actions, expert_actions, rows_out, kept_out=None):
            log.add(self.name, "step", view, learner_actions, expert_actions, rows_out, kept_out)
            rows_out.fill_(0.125)
            self.n_calls += 1

        def close(self):
            log.add(self.name, "close")
    return FakeDagger


@pytest.fixture
def wired(monkeypatch):
    """make_env(**HipVecEnv keywords) -> (env, log, made): test_device_path's fixture with a batch that has an expert buffer, learners that act, and a
    recording dagger handle; `env._build_backend` makes the same backend again, so that seed() runs without a GPU."""
    log, made = Log(), dict(her=[], rollout=[], replay=[], dagger=[])

    class Backend(_TorchBackend):
        def __init__(self, desc, clips, n_envs, env_id0):
            self.torch, self.batch, self.n = torch, ExpertBatch(log), N
            self._host = torch.zeros_like(self.batch.packed)
            v = packed_views(self._host.numpy(), N)
            self.obs, self.term_obs, self.reward, self.info, self.done = v["obs"], v["term_obs"], v["reward"], v["info"], v["done"]
            self.imit = self.sir = self.path = None

    for mod, name, kind in ((rollout, "RolloutBuffer", "rollout"), (replay, "ReplayBuffer", "replay")):
        monkeypatch.setattr(mod, name, fake_buffer(kind, log, made))
    for mod, name, slot, members in ((sac, "SacLearner", "sac", 1), (sac, "SacPopulation", "sac_population", 3), (ppo, "PpoLearner", "ppo", 1),
                                     (ppo, "PpoPopulation", "ppo_population", 3)):
        monkeypatch.setattr(mod, name, fake_learner(slot, log, members))
    monkeypatch.setattr(dagger, "Dagger", fake_dagger(log, made["dagger"]))
    clips = hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300)

    def make_env(expert=True, **kw):
        env = hrg.HipVecEnv(N, env_kwargs=dict(horizon=5, shield_type="OFF", seed=3), clips=clips, backend=Backend, **kw)
        if expert:   # (the constructor refuses expert=... over a backend that is handed in: the descriptor is all the path reads)
            env._expert_desc = NS(cartesian=False)
        monkeypatch.setattr(env, "_build_backend", lambda n: Backend(env._desc, clips, n, 0))
        return env, log, made
    return make_env


# ---- every refusal, by its message
def test_attach_dagger_refusals(wired):
    env, log, made = wired(expert=False)
    env.attach_replay(30)
    env.attach_sac()
    with pytest.raises(NotImplementedError, match=r"attach_dagger: no expert: construct the env with expert=dict\(id=\.\.\., \.\.\.\)"):
        env.attach_dagger(30)
    env._expert_desc, env._imit_alpha = NS(cartesian=False), 0.5
    with pytest.raises(NotImplementedError, match="attach_dagger: imitation_reward: the step's own expert call would advance the expert's noise a second time"):
        env.attach_dagger(30)
    env._imit_alpha = None
    with pytest.raises(ValueError, match="attach_dagger: dict is no table of demonstrations"):
        env.attach_dagger(30, table={})
    assert env.attach_dagger(30) is env.dagger
    env.attach_sac_population(3)
    with pytest.raises(NotImplementedError, match="attach_dagger: env.sac_population: DAgger covers lone learners, not a population"):
        env.attach_dagger(30)
    with pytest.raises(NotImplementedError, match="collect_dagger: env.sac_population: DAgger covers lone learners, not a population"):
        env.collect_dagger(1)
    env.close()
    env, log, made = wired()
    handles = len(made["dagger"])
    with pytest.raises(NotImplementedError, match="collect_dagger: call attach_dagger"):
        env.collect_dagger(1)
    with pytest.raises(NotImplementedError, match="attach_dagger: no learner is attached: DAgger serves one lone learner; call attach_sac .after attach_replay. or attach_ppo"):
        env.attach_dagger(30)
    env.attach_replay(30)
    env.attach_rollout(2)
    env.attach_sac()
    env.attach_ppo()
    with pytest.raises(NotImplementedError, match="attach_dagger: a sac and a ppo learner are attached"):
        env.attach_dagger(30)
    assert env.dagger is None and len(made["dagger"]) == handles   # nothing was made on the way
    env.close()
    env, log, made = wired(monitor_dir=None)
    env.attach_replay(30)
    env.attach_sac()
    env.attach_dagger(30)
    env._monitor = NS(close=lambda: None)
    with pytest.raises(NotImplementedError, match=r"collect_dagger with monitor_dir: the Monitor csv is written by the host path; env.dagger.stats\(\) is the device path's account"):
        env.collect_dagger(1)
    env.close()
    goal, log, made = wired(goal_env=True)
    with pytest.raises(NotImplementedError, match="attach_dagger: goal_env: the scripted experts read flat observations"):
        goal.attach_dagger(30)
    goal.close()
    stub = NS(slices=[slice(0, 2), slice(2, 4)], env_ids=["ReachHuman", "PickPlaceHumanCart"], step_async=None, close=lambda: None)
    with pytest.raises(NotImplementedError, match="attach_dagger: scripted experts are per task and action form; use one HipVecEnv per task"):
        mixed.MixedHipVecEnv(stub).attach_dagger(30)
    clips = hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300)
    ek = dict(shield_type="OFF", horizon=5)
    other = hrg.HipVecEnv(3, env_kwargs=ek, clips=clips, backend=OracleBackend(hrg.build_model_desc(ek, n_clips=2), clips, 3))
    with pytest.raises(NotImplementedError, match="attach_dagger: the dagger kernels run in the HIP library; another backend has none"):
        other.attach_dagger(30)
    other.close()


def test_handle_refusals_come_before_the_library_is_opened(monkeypatch):
    """dagger.Dagger's own checks, which are hrg_dagger_create's: on a machine without a GPU the first thing _open does is raise RuntimeError."""
    low, high = -np.ones(4), np.ones(4)
    new = lambda **kw: dagger.Dagger(**{**dict(kind="sac", n_envs=4, obs_dim=6, act_dim=4, capacity_steps=2, low=low, high=high), **kw})   # noqa: E731
    for obs_dim in (0, 65):
        with pytest.raises(NotImplementedError, match=f"dagger: obs_dim = {obs_dim} outside 1 .. 64"):
            new(obs_dim=obs_dim)
    for act_dim in (0, 8):
        with pytest.raises(NotImplementedError, match=f"dagger: act_dim = {act_dim} outside 1 .. 7"):
            new(act_dim=act_dim, low=-np.ones(act_dim), high=np.ones(act_dim))
    with pytest.raises(ValueError, match="dagger: capacity_steps = 0 must be positive"):
        new(capacity_steps=0)
    with pytest.raises(ValueError, match="dagger: the action bounds must be finite with high > low"):
        new(high=np.array([1.0, 1.0, -1.0, 1.0]))
    with pytest.raises(ValueError, match="dagger: bounds of 3 and 4 values for actions of 4"):
        new(low=-np.ones(3))
    for beta in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="outside .0, 1."):
            new(beta=beta)
    with pytest.raises(ValueError, match="dagger: kind = 'td3'"):
        new(kind="td3")
    table = bc.DemoTable(torch.zeros(5, 6), torch.zeros(5, 4), "ppo")
    with pytest.raises(ValueError, match="dagger: a pinned table of kind 'ppo' for a sac learner"):
        new(pinned=table)
    table = bc.DemoTable(torch.zeros(5, 7), torch.zeros(5, 4), "sac")
    with pytest.raises(ValueError, match="dagger: the pinned table holds observations of 7 and actions of 4 values, the steps write 6 and 4"):
        new(pinned=table)
    table = bc.DemoTable(torch.zeros(5, 6), torch.zeros(5, 4), "sac")
    with pytest.raises(ValueError, match="dagger: the pinned table lives on cpu, the envs on cuda:0"):
        new(pinned=table)


def test_the_table_grows_and_bc_refuses_it_while_empty():
    t = dagger.DaggerTable(torch, "sac", 3, 2, 4, 2, torch.device("cpu"))
    assert isinstance(t, bc.DemoTable) and t.n_rows == 0 and tuple(t.observations.shape) == (6, 2) and tuple(t.actions.shape) == (6, 4)
    for steps, rows in ((1, 3), (2, 6), (5, 6)):
        t.steps = steps
        assert t.n_rows == rows
    pinned = bc.DemoTable(torch.ones(5, 2), torch.full((5, 4), 2.0), "sac")
    t = dagger.DaggerTable(torch, "sac", 3, 2, 4, 2, torch.device("cpu"), pinned)
    assert t.n_rows == t.pinned_rows == 5 and tuple(t.observations.shape) == (11, 2)
    assert bool((t.observations[:5] == 1).all()) and bool((t.actions[:5] == 2).all()) and not t.observations[5:].any()
    t.steps = 1
    assert t.n_rows == 8
    # bc.step on the empty table: the check stands ahead of everything the step does with the device
    step = bc.BehaviourCloning.step
    with pytest.raises(ValueError, match=r"behaviour cloning: the table is empty \(n_rows = 0\)"):
        step(NS(torch=torch, table=dagger.DaggerTable(torch, "sac", 3, 2, 4, 2, torch.device("cpu")), learner=NS(p=None)))
    s = dagger.summarise(np.array([10.0, 4.0, 8.0]), 4, beta=0.5)
    assert s == dict(steps=10, expert_steps=4, sq_error=8.0, expert_fraction=0.4, imitation_error=0.2, beta=0.5)
    assert np.isnan(dagger.summarise(np.zeros(3), 4)["imitation_error"])


# ---- the lifecycle of the path
def test_sac_loop_order_and_what_each_call_is_handed(wired):
    env, log, made = wired(ik_position_delta=dict(action_limit=0.15))
    rb = env.attach_replay(30)
    learner = env.attach_sac()
    dg = env.attach_dagger(30, beta=0.25, seed=11)
    assert dg is env.dagger is made["dagger"][0] and log.names() == ["replay0.new", "sac.new", "dagger0.new"]
    a = dg.args
    assert (a["kind"], a["n_envs"], a["obs_dim"], a["act_dim"], a["capacity_steps"], a["seed"], a["pinned"], dg.beta) == ("sac", N, rb.obs_dim, 4, 10, 11, None, 0.25)
    np.testing.assert_array_equal(a["low"], env.action_space.low)
    assert env.attach_dagger(2).args["capacity_steps"] == 1 and env.dagger.args["seed"] == 3   # max(capacity // num_envs, 1); the env's seed
    assert log.names(3) == ["dagger1.new", "dagger0.close"] and env.dagger is made["dagger"][1]   # attaching again replaces the handle
    step = ["sac.act", "batch.expert_actions", "dagger1.step", "batch.step", "replay0.add_step"]
    at = len(log)
    assert env.collect_dagger(2) is env.dagger
    assert log.names(at) == ["batch.reset", "replay0.observe"] + step + step
    at = len(log)
    env.collect_dagger(1, deterministic=False)
    assert log.names(at) == step   # the second call continues
    view, learner_actions, expert, rows, kept = log.last("dagger1.step").args
    assert log.last("sac.act").args[0] is view and log.last("sac.act").args[1] is False
    assert learner_actions is learner.actions and expert is env._backend.batch._expert_act
    assert rows.dtype == torch.float64 and tuple(rows.shape) == (N, ACT) and kept.dtype == torch.float32 and tuple(kept.shape) == (N, 4)
    sent, before = log.last("batch.step").args
    assert sent is rows and bool((before == 0.125).all())   # the rows the dagger step wrote are the rows the envs execute
    assert log.last("replay0.add_step").args[0] is kept   # and what it kept is what the buffer stores
    with pytest.raises(RuntimeError, match="step_async after collect_dagger"):
        env.step_async(np.zeros((N, 4)))
    at = len(log)
    env.reset()
    env.step(np.zeros((N, 4)))
    assert log.names(at) == ["batch.reset", "replay0.observe", "batch.step", "replay0.add_step"]
    at = len(log)
    env.collect_dagger(1)
    assert log.names(at) == ["batch.reset", "replay0.observe"] + step   # after reset() the loop starts from its own reset again
    env.close()


def test_ppo_loop_keeps_the_rollout_rows_in_step_and_fills_no_slot(wired):
    env, log, made = wired()
    env.attach_rollout(2)
    env.attach_ppo()
    env.attach_dagger(30)
    assert made["dagger"][0].args["kind"] == "ppo" and made["dagger"][0].args["act_dim"] == ACT
    step = ["ppo.policy", "batch.expert_actions", "dagger0.step", "batch.step", "rollout0.observe"]
    at = len(log)
    env.collect_dagger(2)
    assert log.names(at) == ["batch.reset", "rollout0.observe"] + step + step
    assert log.last("dagger0.step").args[4] is None and log.last("ppo.policy").args[1] is True
    assert log.last("rollout0.observe").args == (env._backend.batch.obs,)
    at = len(log)
    env.collect_dagger(1)
    assert log.names(at) == step   # continues: the buffer's current rows followed the envs
    at = len(log)
    env.collect_rollout(env.ppo.policy, lambda obs: torch.zeros(N))
    assert log.names(at)[:3] == ["batch.reset", "rollout0.observe", "rollout0.reset"]   # the on-policy loop starts from a reset: its episode flags saw none of these steps
    assert "rollout0.add_step" not in log.names(0)[:at]
    at = len(log)
    env.collect_dagger(1)
    assert log.names(at) == step   # (and a rollout leaves the rows where the next dagger step finds them)
    env.close()


def test_seed_rebuilds_the_handle_empty_and_close_closes_it(wired):
    env, log, made = wired()
    env.attach_replay(30)
    env.attach_sac()
    pinned = NS(kind="sac", n_rows=5)
    env.attach_dagger(30, beta=0.75, table=pinned, seed=9)
    first = env.dagger
    env._device_path.bc = cloning = NS(table=first.table, learner=env.sac, close=lambda: log.add("bc", "close"))
    env.collect_dagger(1)
    first.beta = 0.1   # (a schedule's value is not an argument of attach)
    at = len(log)
    env.seed(4)
    assert log.names(at) == ["replay0.close", "batch.close", "replay1.new", "dagger1.new", "dagger0.close"]
    new = env.dagger
    assert new is made["dagger"][1] is not first and new.n_calls == 0 and new.beta == 0.75 and new.args["pinned"] is pinned and new.args["seed"] == 9
    assert cloning.table is new.table   # the attached cloning goes on, on the new table
    at = len(log)
    env.collect_dagger(1)
    assert log.names(at) == ["batch.reset", "replay1.observe", "sac.act", "batch.expert_actions", "dagger1.step", "batch.step", "replay1.add_step"]
    at = len(log)
    env.close()
    assert log.names(at) == ["bc.close", "dagger1.close", "sac.close", "replay1.close", "batch.close"]
    assert env.dagger is None


# ---- the tools
def _tool(name):
    spec = importlib.util.spec_from_file_location("tool_" + name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_parsers():
    ap = _tool("train_dagger").ap
    a = ap.parse_args(["--env", "ReachHuman", "--out", "models/dagger/model_final.npz"])
    assert (a.algorithm, a.iterations, a.collect_steps, a.bc_steps, a.beta0, a.decay, a.critic_steps, a.seed_dataset, a.eval_episodes) == ("sac", 10, 100, 500, 0.5, 0.7, 0, None, 0)
    a = ap.parse_args(["--env", "ReachHuman", "--out", "o.npz", "--algorithm", "ppo", "--seed-dataset", "reach-demo", "--beta0", "1", "--decay", "0.5", "--critic-steps", "3"])
    assert (a.algorithm, a.seed_dataset, a.beta0, a.decay, a.critic_steps) == ("ppo", "reach-demo", 1.0, 0.5, 3)
    assert [_tool("train_dagger").beta_of(a, i) for i in range(3)] == [1.0, 0.5, 0.25]
    with pytest.raises(SystemExit):
        ap.parse_args(["--env", "ReachHuman", "--out", "o.npz", "--algorithm", "td3"])
    b = _tool("bench_dagger").ap.parse_args([])
    assert (b.n_envs, b.steps, b.blocks, b.out) == (1024, 100, 8, "profiles/r32_dagger.json")
