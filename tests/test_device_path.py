"""The lifecycle of the device training path (device_path.DevicePath behind HipVecEnv) without a GPU: when the envs are reset, when each buffer is handed rows,
what it stores, when step_async refuses, what close() closes -- as the order of calls on a recording batch and recording buffers, with tensor identity,
dtype and values where they matter.  The expected sequences were recorded on the commit before the device path got its owner, with the same fakes wired
into that commit's backend (the `wired` fixture is the only part that differed), so they state what the env did before as well as what it does now.

Left to GPU tests, because seed() rebuilds a real batch: test_rollout_gpu.py::test_collect_rollout_refusals_and_reseeding and
test_replay_gpu.py::test_attach_replay_refusals_and_reseeding."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import human_robot_gym_amd as hrg
from human_robot_gym_amd import evaluation, her, ppo, replay, rollout, sac
from human_robot_gym_amd._cstruct import CONST
from human_robot_gym_amd.dist import packed_layout, packed_views
from human_robot_gym_amd.vec_env import _TorchBackend

N = 3
IK = dict(action_limit=0.15)


class Log(list):
    def add(self, who, what, *args, **kwargs):
        self.append(NS(name=f"{who}.{what}", args=args, kwargs=kwargs))

    def names(self, start=0):
        return [e.name for e in self[start:]]

    def last(self, name):
        return [e for e in self if e.name == name][-1]


class FakeBatch:
    """The calls of a HipBatch the env makes, recorded; the outputs are small CPU tensors.  A step rewrites its action rows, like the kernel's front-ends."""

    def __init__(self, log):
        self.log, self.n, self.device = log, N, torch.device("cpu")
        self.packed = torch.zeros(packed_layout(N)["total"], dtype=torch.uint8)
        for k, v in packed_views(self.packed, N).items():
            setattr(self, k, v)

    def reset(self):
        self.log.add("batch", "reset")
        self.obs.zero_()

    dataset_reset = reset

    def step(self, act):
        self.log.add("batch", "step", act, act.clone())
        act.mul_(0.5)
        self.obs.add_(1.0)

    step_imitation = step_dataset = step

    def close(self):
        self.log.add("batch", "close")


def fake_buffer(kind, log, made):
    class FakeBuffer:
        """Stands in for her.HerBuffer / rollout.RolloutBuffer / replay.ReplayBuffer: the sizes of the descriptor, every call recorded under <kind><k>."""

        def __init__(self, desc, device=0, info_keys=None):
            self.name = f"{kind}{len(made[kind])}"
            made[kind].append(self)
            self.n, self.act_dim, self.obs_dim, self.device = int(desc.n_envs), int(desc.act_dim), int(desc.n_obs_cols), torch.device("cpu")
            self.n_steps, self.observe_time, self.obs_features = int(getattr(desc, "n_steps", 0)), False, int(desc.n_obs_cols)
            log.add(self.name, "new", device, info_keys)

        def observation(self):
            return torch.zeros(self.n, self.obs_dim)

        def view(self, rows):
            log.add(self.name, "view", rows)
            return rows[:, :self.obs_dim]

    for what in ("observe", "add_step", "reset", "compute_returns_and_advantage", "close"):
        setattr(FakeBuffer, what, lambda self, *a, _what=what, **k: log.add(self.name, _what, *a, **k))
    return FakeBuffer


def fake_learner(slot, log):
    class FakeLearner:
        _shared = {}

        def __init__(self, *args, **kwargs):
            log.add(slot, "new")

        def close(self):
            log.add(slot, "close")
    return FakeLearner


class FakeEvaluator:
    max_quota = 1

    def __init__(self, desc, device=0, info_keys=None):
        FakeEvaluator.log.add("eval", "new")

    def policy(self, learner, params=None):
        self.log.add("eval", "policy")
        return torch.zeros(N, CONST["HRG_ACT_DIM"], dtype=torch.float64)

    def remaining(self):
        self.log.add("eval", "remaining")
        return 0


for _what in ("begin", "step", "result", "close"):
    setattr(FakeEvaluator, _what, lambda self, *a, _what=_what, **k: self.log.add("eval", _what, *a, **k))


@pytest.fixture
def wired(monkeypatch):
    """make_env(**HipVecEnv keywords) -> (env, log, made): an env over a _TorchBackend whose constructor alone is replaced (a FakeBatch, a CPU tensor for the host
    block), with the recording buffers, learners and evaluator in place of the real classes."""
    log, made = Log(), dict(her=[], rollout=[], replay=[])

    class Backend(_TorchBackend):
        def __init__(self, desc, clips, n_envs, env_id0):
            self.torch, self.batch, self.n = torch, FakeBatch(log), N
            self._host = torch.zeros_like(self.batch.packed)
            v = packed_views(self._host.numpy(), N)
            self.obs, self.term_obs, self.reward, self.info, self.done = v["obs"], v["term_obs"], v["reward"], v["info"], v["done"]
            self.imit = self.sir = self.path = None

    for mod, name, kind in ((her, "HerBuffer", "her"), (rollout, "RolloutBuffer", "rollout"), (replay, "ReplayBuffer", "replay")):
        monkeypatch.setattr(mod, name, fake_buffer(kind, log, made))
    for mod, name, slot in ((sac, "SacLearner", "sac"), (sac, "SacPopulation", "sac_population"), (ppo, "PpoLearner", "ppo"), (ppo, "PpoPopulation", "ppo_population")):
        monkeypatch.setattr(mod, name, fake_learner(slot, log))
    FakeEvaluator.log = log
    monkeypatch.setattr(evaluation, "Evaluator", FakeEvaluator)
    clips = hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300)

    def make_env(**kw):
        return hrg.HipVecEnv(N, env_kwargs=dict(horizon=5, shield_type="OFF", seed=3), clips=clips, backend=Backend, **kw), log, made
    return make_env


def bounds(env):
    return np.asarray(env.action_space.low, np.float64), np.asarray(env.action_space.high, np.float64)


def policy_scale(env, a):
    low, high = bounds(env)
    return (2.0 * ((np.asarray(a, np.float64) - low) / (high - low)) - 1.0).astype(np.float32)


class Policy:
    """A fixed action tensor as the policy of collect_steps; every call recorded."""

    def __init__(self, log, A, value=0.5):
        self.log, self.actions = log, torch.full((N, A), value, dtype=torch.float32)

    def __call__(self, obs):
        self.log.add("policy", "act", obs)
        return self.actions


def widened(a):
    rows = np.zeros((N, CONST["HRG_ACT_DIM"]))
    rows[:, :a.shape[1]] = a
    return rows


# ---- 1 and 2: the host path fills the replay buffer ----
def test_replay_attached_before_reset_is_filled_by_reset_and_step(wired):
    env, log, made = wired(ik_position_delta=IK)
    low, high = bounds(env)
    assert high[0] == np.float32(0.15) and low[3] == -1.0   # bounds that are not +-1: the scaling is visible
    rb = env.attach_replay(30)
    assert env.replay is rb is made["replay"][0] and log.names() == ["replay0.new"] and log[0].args == (None, env._info_keys)
    env.reset()
    assert log.names(1) == ["batch.reset", "replay0.observe"]
    assert log[-1].args[0] is env._backend.batch.obs and log[-1].kwargs == dict(time=None)
    rng = np.random.RandomState(0)
    for k in range(2):
        at = len(log)
        a = rng.uniform(low, high, (N, 4))
        env.step(a)
        assert log.names(at) == ["batch.step", "replay0.add_step"]
        b = env._backend.batch
        stored, *rest = log[-1].args
        assert stored.dtype == torch.float32 and stored.is_contiguous() and log[-1].kwargs == {}
        np.testing.assert_array_equal(stored.numpy(), policy_scale(env, a))
        assert all(x is y for x, y in zip(rest, (b.obs, b.term_obs, b.reward, b.done, b.info)))
        sent = log[at].args[1]
        assert sent.dtype == torch.float64
        np.testing.assert_array_equal(sent.numpy(), widened(a))   # [dx, dy, dz, gripper, 0, 0, 0]
    env.close()


def test_replay_attached_in_mid_run_observes_the_rows_on_the_device(wired):
    env, log, made = wired(ik_position_delta=IK)
    env.reset()
    env.step(np.zeros((N, 4)))
    at = len(log)
    env.attach_replay(30)
    assert log.names(at) == ["replay0.new", "replay0.observe"] and log[-1].args[0] is env._backend.batch.obs   # no reset
    env.step(np.zeros((N, 4)))
    assert log.names(at + 2) == ["batch.step", "replay0.add_step"]
    env.close()


# ---- 3: the device loop and a re-attach ----
def test_collect_steps_resets_once_and_a_reattach_restarts(wired):
    env, log, made = wired(ik_position_delta=IK)
    low, high = bounds(env)
    rb = env.attach_replay(30)
    pol = Policy(log, 4)
    step = ["policy.act", "batch.step", "replay0.add_step"]
    assert env.collect_steps(pol, 2) is rb
    assert log.names(1) == ["batch.reset", "replay0.observe"] + step + step
    at = len(log)
    env.collect_steps(pol, 2)
    assert log.names(at) == step + step   # the second call continues
    assert log[-1].args[0] is pol.actions   # the policy's own float32 action
    sent = log[-2].args[1]
    assert sent.dtype == torch.float64
    np.testing.assert_array_equal(sent.numpy(), widened(low + 0.5 * (pol.actions.numpy().astype(np.float64) + 1.0) * (high - low)))
    with pytest.raises(RuntimeError, match="step_async after collect_steps"):
        env.step_async(np.zeros((N, 4)))
    at = len(log)
    assert env.attach_replay(40) is made["replay"][1] is env.replay
    assert log.names(at) == ["replay0.close", "replay1.new", "batch.reset", "replay1.observe"]   # between two runs of the loop: the envs start again
    with pytest.raises(RuntimeError, match="step_async after collect_steps"):
        env.step_async(np.zeros((N, 4)))
    at = len(log)
    env.reset()
    env.step(np.zeros((N, 4)))
    assert log.names(at) == ["batch.reset", "replay1.observe", "batch.step", "replay1.add_step"]
    env.close()


# ---- 4: the same for the hindsight buffer on a goal env ----
@pytest.mark.parametrize("ik", [None, IK])
def test_her_on_the_host_path_and_in_the_device_loop(wired, ik):
    env, log, made = wired(goal_env=True, ik_position_delta=ik)
    A = env.action_space.shape[0]
    low, high = bounds(env)
    hb = env.attach_her(30)
    assert env.her is hb and log.names() == ["her0.new"]
    env.reset()
    assert log.names(1) == ["batch.reset", "her0.observe"] and log[-1].args == (env._backend.batch.obs,) and log[-1].kwargs == {}
    a = np.random.RandomState(1).uniform(low, high, (N, A))
    at = len(log)
    env.step(a)
    assert log.names(at) == ["batch.step", "her0.add_step"]
    received, before = log[at].args
    stored = log[-1].args[0]
    assert stored.dtype == torch.float64 and log[-1].kwargs == {}
    if ik is None:
        assert stored is received   # the rows as the step left them
    else:   # behind the IK front-end: the rows the agent sent, copied before the step rewrote them
        assert stored is not received and torch.equal(stored, before) and not torch.equal(stored, received)
    env.close()
    # attached in mid-run; then the device loop, twice; then attached again
    env, log, made = wired(goal_env=True, ik_position_delta=ik)
    del log[:]
    env.reset()
    env.step(np.zeros((N, A)))
    at = len(log)
    hb = env.attach_her(30)
    assert log.names(at) == [f"{hb.name}.new", f"{hb.name}.observe"]
    pol = Policy(log, A)
    step = ["policy.act", "batch.step", f"{hb.name}.add_step"]
    at = len(log)
    assert env.collect_steps(pol, 2) is hb
    assert log.names(at) == ["batch.reset", f"{hb.name}.observe"] + step + step
    at = len(log)
    env.collect_steps(pol, 2)
    assert log.names(at) == step + step
    received, before = log[-2].args
    stored = log[-1].args[0]
    np.testing.assert_array_equal(before.numpy(), widened(low + 0.5 * (pol.actions.numpy().astype(np.float64) + 1.0) * (high - low)))
    if ik is None:
        assert stored is received
    else:
        assert stored is not received and torch.equal(stored, before)
    at = len(log)
    new = env.attach_her(31)
    assert log.names(at) == [f"{hb.name}.close", f"{new.name}.new", "batch.reset", f"{new.name}.observe"]
    with pytest.raises(RuntimeError, match="step_async after collect_steps"):
        env.step_async(np.zeros((N, A)))
    env.reset()
    env.step(np.zeros((N, A)))
    assert log.names()[-2:] == ["batch.step", f"{new.name}.add_step"]
    env.close()


# ---- 5: the rollout loop ----
def test_collect_rollout_resets_once_and_sends_clipped_widened_rows(wired):
    env, log, made = wired(ik_position_delta=IK)
    rb = env.attach_rollout(2)
    actions = torch.tensor([[0.3, -0.3, 0.1, 2.0]] * N, dtype=torch.float32)   # outside the bounds +-0.15 and +-1

    def policy(obs):
        log.add("policy", "act")
        return actions, torch.zeros(N), torch.zeros(N)

    def value(obs):
        log.add("value", "of")
        return torch.zeros(N)

    step = ["policy.act", "batch.step", "rollout0.view", "value.of", "rollout0.add_step"]
    assert env.collect_rollout(policy, value) is rb
    assert log.names(1) == ["batch.reset", "rollout0.observe", "rollout0.reset"] + step + step + ["value.of", "rollout0.compute_returns_and_advantage"]
    at = len(log)
    env.collect_rollout(policy, value)
    assert log.names(at) == ["rollout0.reset"] + step + step + ["value.of", "rollout0.compute_returns_and_advantage"]
    sent = log.last("batch.step").args[1]
    low, high = env.action_space.low, env.action_space.high
    assert sent.dtype == torch.float64
    np.testing.assert_array_equal(sent.numpy(), widened(np.clip(actions.numpy(), low, high)))   # clamped in float32, then widened with zeros
    assert log.last("rollout0.add_step").args[0] is actions   # the buffer stores what the policy emitted
    assert log.last("rollout0.view").args[0] is env._backend.batch.term_obs
    with pytest.raises(RuntimeError, match="step_async after collect_rollout"):
        env.step_async(np.zeros((N, 4)))
    env.close()


def test_attach_rollout_between_two_loops_restarts_for_every_attached_buffer(wired):
    """The one sequence that is not the earlier commit's: there attach_rollout reset the batch itself and handed the rows to the new rollout buffer alone
    (recorded: rollout0.close, rollout1.new, batch.reset, rollout1.observe); now it is the restart of the other two attaches, and a replay buffer attached
    next to it gets the reset's rows too."""
    env, log, made = wired()
    env.attach_replay(30)
    env.attach_rollout(2)
    env.collect_rollout(lambda obs: (torch.zeros(N, 7), torch.zeros(N), torch.zeros(N)), lambda obs: torch.zeros(N))
    at = len(log)
    env.attach_rollout(2)
    assert log.names(at) == ["rollout0.close", "rollout1.new", "batch.reset", "replay0.observe", "rollout1.observe"]
    env.close()


# ---- 6: an evaluation leaves the buffers behind ----
def test_evaluate_starts_from_a_reset_and_the_next_loop_resets_again(wired):
    env, log, made = wired(ik_position_delta=IK)
    env.attach_replay(30)
    pol = Policy(log, 4)
    env.collect_steps(pol, 1)
    at = len(log)
    learner = NS(p=NS(n_params=1), _prefix="hrg_sac")
    env.evaluate(learner, n_eval_episodes=1, sync_every=1)
    assert log.names(at) == ["batch.reset", "replay0.observe", "eval.new", "eval.begin", "eval.policy", "batch.step", "eval.step", "eval.remaining", "eval.result",
                             "eval.close"]   # no add_step: the buffer sees none of the evaluation's steps
    with pytest.raises(RuntimeError, match="step_async after evaluate"):
        env.step_async(np.zeros((N, 4)))
    at = len(log)
    env.collect_steps(pol, 1)
    assert log.names(at) == ["batch.reset", "replay0.observe", "policy.act", "batch.step", "replay0.add_step"]
    at = len(log)
    env.collect_steps(pol, 1)
    assert log.names(at) == ["policy.act", "batch.step", "replay0.add_step"]
    env.close()


# ---- 7: close ----
def test_close_closes_every_buffer_and_learner_once_and_then_the_batch(wired):
    env, log, made = wired()
    env.attach_rollout(8)
    env.attach_replay(30)
    env.attach_sac()
    env.attach_sac_population(3)
    env.attach_ppo()
    env.attach_ppo_population(3, batch_size=8)
    assert log.names() == ["rollout0.new", "replay0.new", "sac.new", "sac_population.new", "ppo.new", "ppo_population.new"]
    env.attach_sac()   # the previous learner of the slot is closed
    assert log.names(6) == ["sac.new", "sac.close"]
    at = len(log)
    env.close()
    assert log.names(at) == ["sac.close", "sac_population.close", "ppo.close", "ppo_population.close", "rollout0.close", "replay0.close", "batch.close"]
