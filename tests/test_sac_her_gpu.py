"""SAC + HER on the device: the fused feature sampler against tests/her_ref.py and against `sample()`, the feature view, the episode statistics of the
hindsight buffer, `collect_steps` into it against the host's reset / step loop, and the learner on top.  -m gpu.

Sizes are test_her_gpu's: 4 envs with rings of 16 slots, horizon 6, 45 steps (the rings wrap, goal slots cross the seam, env 3 never closes an episode), sample
batches of 1, 63, 65 and 257 (four samples per 256-thread block: a block with one wave, a block short of one wave, full blocks and a last block with one wave).
Feature rows of 45 (reach) and 40 (cube) values: neither a multiple of anything the kernels tile by.  The env tests: 64 envs, horizon 4."""
import math

import numpy as np
import pytest

import her_ref as R
import human_robot_gym_amd as hrg
from human_robot_gym_amd._cstruct import CONST
from test_her_gpu import DG_IN_OBS, OBS_COLS, PARAMS, _assert_ring_equal, _buffer, _dev, _filled, _mask

pytestmark = pytest.mark.gpu

FEATURE_COLS = {kind: R.AG_COLS[kind] + R.DG_COLS[kind] + OBS_COLS[kind] for kind in OBS_COLS}   # the feature row of a stored row, where no goal was relabelled
BATCHES = (1, 63, 65, 257)


def _want_features(want):
    """achieved_goal | desired_goal | observation of her_ref's sample, both rows."""
    return (np.concatenate([want["achieved_goal"], want["desired_goal"], want["observation"]], axis=1),
            np.concatenate([want["next_achieved_goal"], want["next_desired_goal"], want["next_observation"]], axis=1))


def _assert_features_equal(buf, got, want, what):
    f0, f1 = _want_features(want)
    np.testing.assert_array_equal(buf.last_index.cpu().numpy(), want["index"], err_msg=f"{what}: index")
    np.testing.assert_array_equal(got.observations.cpu().numpy(), f0, err_msg=f"{what}: features")
    np.testing.assert_array_equal(got.next_observations.cpu().numpy(), f1, err_msg=f"{what}: next features")
    np.testing.assert_array_equal(got.actions.cpu().numpy(), want["action"], err_msg=f"{what}: action")
    np.testing.assert_array_equal(got.dones.cpu().numpy(), want["done"], err_msg=f"{what}: done")
    np.testing.assert_allclose(got.rewards.cpu().numpy(), want["reward"], rtol=1e-6, atol=1e-6, err_msg=f"{what}: reward")


def _cat(d):
    import torch
    return torch.cat([d["achieved_goal"], d["desired_goal"], d["observation"]], dim=1)


def _assert_same_batch(dict_batch, flat_batch, rows=None):
    """A DictReplayBufferSamples, concatenated, and a ReplayBufferSamples: bit-equal in every output (the first `rows` rows)."""
    pairs = ((_cat(dict_batch.observations), flat_batch.observations), (_cat(dict_batch.next_observations), flat_batch.next_observations),
             (dict_batch.actions, flat_batch.actions), (dict_batch.rewards, flat_batch.rewards), (dict_batch.dones, flat_batch.dones))
    for k, (x, y) in enumerate(pairs):
        np.testing.assert_array_equal(x.cpu().numpy()[:rows], y.cpu().numpy()[:rows], err_msg=f"output {k}")


@pytest.mark.parametrize("kind", ["reach", "cube"])
@pytest.mark.parametrize("strategy", ["future", "final", "episode"])
def test_feature_samples_are_the_references(oracle_lib, kind, strategy):
    """Batches of 1, 63, 65 and 257 at her_ratio 0, 0.8 and 1: the feature rows are concat(achieved_goal, desired_goal, observation) of her_ref's sample,
    bit-equal with the actions, done flags and the index; rewards at rtol 1e-6 / atol 1e-6 (FP64 with the device's approximate sqrt), no compared sample
    within 1e-6 of the success threshold."""
    u01 = oracle_lib.hrgo_test_u01
    relabelled = kept = 0
    for ratio in (0.0, 0.8, 1.0):
        buf, ring = _filled(kind, strategy, ratio)
        buf.record_index = True
        assert buf.obs_features == len(FEATURE_COLS[kind]) == {"reach": 45, "cube": 40}[kind]
        for call, B in enumerate(BATCHES):
            want = R.sample(ring, u01, 11, call, B, kind, ratio, strategy, params=PARAMS[kind], obs_cols=OBS_COLS[kind])
            assert want["margin"].min() >= 1e-6   # a threshold flip cannot hide in the reward tolerance
            assert buf.counts_host()[2] == call
            got = buf.sample_features(B)
            assert got.observations.shape == got.next_observations.shape == (B, buf.obs_features) and got.rewards.shape == got.dones.shape == (B, 1)
            _assert_features_equal(buf, got, want, f"{kind} {strategy} ratio {ratio} batch {B}")
            assert np.all(want["index"][:, 0] != 3)   # the env without a closed transition
            rl = want["relabel"]
            relabelled += int(rl.sum())
            kept += int((~rl).sum())
            # a sample that kept its goal is the stored rows' columns
            e, i = want["index"][~rl, 0], want["index"][~rl, 1]
            np.testing.assert_array_equal(got.observations.cpu().numpy()[~rl], ring.pre[e, i % ring.cap][:, FEATURE_COLS[kind]])
        assert buf.counts_host()[2] == len(BATCHES)
        buf.close()
    assert relabelled > 300 and kept > 300


@pytest.mark.parametrize("kind", ["reach", "cube"])
def test_feature_samples_with_relabel_observation(oracle_lib, kind):
    """relabel_observation: the copy of the goal inside the observation entry moves with it, behind the two goal entries of the row."""
    buf, ring = _filled(kind, relabel_observation=True)
    buf.record_index = True
    want = R.sample(ring, oracle_lib.hrgo_test_u01, 11, 0, 257, kind, 0.8, params=PARAMS[kind], obs_cols=OBS_COLS[kind], relabel_observation=True, dg_in_obs=DG_IN_OBS[kind])
    assert want["margin"].min() >= 1e-6
    got = buf.sample_features(257)
    _assert_features_equal(buf, got, want, f"{kind} relabel_observation")
    sl = buf.feature_slices()
    f = got.observations.cpu().numpy()
    at = [sl["observation"].start + c for c in DG_IN_OBS[kind]]
    np.testing.assert_array_equal(f[:, at][want["relabel"]], f[:, sl["desired_goal"]][want["relabel"]])
    assert 0 < want["relabel"].sum() < 257
    buf.close()


def test_feature_samples_are_sample_concatenated():
    """Two buffers filled alike, at the same call counter: sample(B) concatenated and sample_features(B) are bit-equal in every output, rewards included.
    Interleaved calls on one buffer advance one counter; the first 65 rows of a 257-row call are a 65-row call."""
    for kind in ("reach", "cube"):
        (a, _), (b, _) = _filled(kind), _filled(kind)
        a.record_index = b.record_index = True
        for call, B in enumerate(BATCHES):
            assert a.counts_host()[2] == b.counts_host()[2] == call
            _assert_same_batch(a.sample(B), b.sample_features(B))
            np.testing.assert_array_equal(a.last_index.cpu().numpy(), b.last_index.cpu().numpy())
        # from here on a and b swap roles on every call: one counter behind both entry points
        for call, B in enumerate((65, 63, 257), start=len(BATCHES)):
            da, fb = (a.sample(B), b.sample_features(B)) if call % 2 else (b.sample(B), a.sample_features(B))
            _assert_same_batch(da, fb)
            assert a.counts_host()[2] == b.counts_host()[2] == call + 1
        big, small = a.sample_features(257), b.sample_features(65)
        for x, y in zip(big, small):
            np.testing.assert_array_equal(x.cpu().numpy()[:65], y.cpu().numpy())
        np.testing.assert_array_equal(a.last_index.cpu().numpy()[:65], b.last_index.cpu().numpy())
        # the prefix sums are cached until the counts change: a step that closes episodes changes what the next call draws from
        closed = a.size()
        step = list(R.scripted_steps(4, 1, 6, seed=9, p_done=1.0))[0]
        for buf in (a, b):
            buf.add_step(*_dev(step))
        assert a.size() > closed
        _assert_same_batch(a.sample(257), b.sample_features(257))
        np.testing.assert_array_equal(a.last_index.cpu().numpy(), b.last_index.cpu().numpy())
        assert int(a.last_index[:, 0].max()) == 3   # env 3 has closed transitions now, and the cached sums were dropped
        a.close()
        b.close()


@pytest.mark.parametrize("kind", ["reach", "cube"])
def test_the_feature_view_is_the_column_selection(kind):
    """observation() of given rows (1, 5 and 9 rows: one wave, a block and a wave, two blocks and a wave) and of the current rows, after the first observe,
    after a step that finished some envs, and after a masked observe."""
    n = 5
    buf = _buffer(n, 16, 6, kind=kind)
    cols = FEATURE_COLS[kind]
    assert list(buf.feature_slices()) == ["achieved_goal", "desired_goal", "observation"]
    assert [s.stop - s.start for s in buf.feature_slices().values()] == [len(R.AG_COLS[kind]), len(R.DG_COLS[kind]), len(OBS_COLS[kind])]
    rng = np.random.RandomState(7)
    for m in (1, 5, 9):
        rows = rng.uniform(-1, 1, (m, 64)).astype(np.float32)
        got = buf.observation(_dev([rows])[0])
        assert got.shape == (m, buf.obs_features)
        np.testing.assert_array_equal(got.cpu().numpy(), rows[:, cols])
    first = rng.uniform(-1, 1, (n, 64)).astype(np.float32)
    buf.observe(_dev([first])[0])
    np.testing.assert_array_equal(buf.observation().cpu().numpy(), first[:, cols])
    step = list(R.scripted_steps(n, 1, 6, seed=3))[0]
    step[4][:] = [1, 0, 1, 0, 0]
    buf.add_step(*_dev(step))
    np.testing.assert_array_equal(buf.observation().cpu().numpy(), step[1][:, cols])   # (where done: the new episode's first row, not the terminal one)
    again = rng.uniform(-1, 1, (n, 64)).astype(np.float32)
    mask = np.array([0, 1, 1, 0, 1], np.uint8)
    buf.observe(_dev([again])[0], _mask(mask))
    np.testing.assert_array_equal(buf.observation().cpu().numpy(), np.where(mask[:, None] != 0, again, step[1])[:, cols])
    with pytest.raises(ValueError, match="expected a contiguous"):
        buf.observation(_dev([first[:, :63]])[0])
    buf.close()


def test_episode_statistics_of_the_scripted_steps():
    """test_her_gpu._filled's recipe with a tally beside it: episodes, float64 return sums, lengths and the info columns of the last steps, per env.  Env 3 is
    observed again (masked) before every time limit and never finishes: it contributes nothing, and its running sums start again.  `clear` clears; the rings
    are her_ref's as before."""
    n, cap, horizon, n_info = 4, 16, 6, CONST["HRG_INFO_DIM"]
    buf, ring = _buffer(n, cap, horizon), R.Ring(n, cap)
    assert buf._stats_dim == 3 + n_info
    zero = np.zeros((n, 64), np.float32)
    buf.observe(_dev([zero])[0])
    ring.observe(zero)
    tally, run_ret, run_len = np.zeros((n, 3 + n_info)), np.zeros(n), np.zeros(n, np.int64)
    for step in R.scripted_steps(n, 45, horizon, seed=2):
        step[4][3] = 0
        if ring.w[3] - ring.open[3] == horizon - 1:
            m = np.array([0, 0, 0, 1], np.uint8)
            buf.observe(_dev([step[1]])[0], _mask(m))
            ring.observe(step[1], m)
            run_ret[3], run_len[3] = 0.0, 0
        buf.add_step(*_dev(step))
        ring.add(*step)
        _, _, _, reward, done, info = step
        run_ret += reward.astype(np.float64)
        run_len += 1
        for e in np.nonzero(done)[0]:
            tally[e] += np.concatenate([[1.0, run_ret[e], run_len[e]], info[e].astype(np.float64)])
            run_ret[e], run_len[e] = 0.0, 0
    assert np.all(tally[:3, 0] >= 5) and np.all(tally[3] == 0) and tally[:, 3:].any()
    got = buf.episode_stats_per_env(clear=False)
    np.testing.assert_array_equal(got, tally)
    np.testing.assert_array_equal(buf.episode_stats_per_env(clear=False), tally)   # reading without clear changes nothing
    tot = buf.episode_stats(clear=True)
    assert tot["episodes"] == int(tally[:, 0].sum()) and tot["l"] == int(tally[:, 2].sum()) and tot["r"] == float(tally.sum(axis=0)[1])
    assert [tot[k] for k in buf.info_keys] == list(tally.sum(axis=0)[3:]) and len(buf.info_keys) == n_info
    np.testing.assert_array_equal(buf.episode_stats_per_env(), 0.0)
    _assert_ring_equal(buf, ring, "after the scripted steps")   # the tracker sits beside the ring: what hrg_her_export returns did not change
    # the running sums survive the clear: the episode env 0 is in ends with the whole of its return
    step = list(R.scripted_steps(n, 1, horizon, seed=5, p_done=1.0))[0]
    buf.add_step(*_dev(step))
    want = np.stack([np.concatenate([[1.0, run_ret[e] + np.float64(step[3][e]), run_len[e] + 1], step[5][e].astype(np.float64)]) for e in range(n)])
    np.testing.assert_array_equal(buf.episode_stats_per_env(), want)
    buf.close()


ENV_KW = dict(horizon=4, seed=11, shield_type="OFF")
REACH_KEYS = ["object-state", "robot0_joint_pos"]                            # 18 columns: F = 6 + 6 + 18
CUBE_KEYS = ["object_gripped", "vec_eef_to_object", "vec_eef_to_target"]    # 7 columns: F = 7 + 3 + 7


def _goal_env(ik=False, obs_keys=None, n=64):
    kw = dict(goal_env=True, env_kwargs=dict(ENV_KW), clips=hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300))
    if ik:
        return hrg.HipVecEnv(n, env_id="PickPlaceHumanCart", obs_keys=CUBE_KEYS if obs_keys is None else obs_keys, ik_position_delta=dict(action_limit=0.15), **kw)
    return hrg.HipVecEnv(n, obs_keys=REACH_KEYS if obs_keys is None else obs_keys, **kw)


@pytest.mark.parametrize("front_end", ["none", "ik"])
def test_collect_steps_fills_the_rings_like_reset_and_step(front_end):
    """Two envs of 64 goal envs, horizon 4, rings of 40 slots, the same deterministic policy (tanh of a fixed linear map of the feature row): 9 steps of
    collect_steps on one, reset() and 9 x step() on the other, fed the concatenated dict observation.  Every env's ring, the counts and the episode sums are
    equal.  Behind the IK front-end the buffer keeps a copy of the agent's rows.  Afterwards step_async raises until reset()."""
    import torch
    ik = front_end == "ik"
    dev_env, host_env = _goal_env(ik), _goal_env(ik)
    hd, hh = dev_env.attach_her(40), host_env.attach_her(40)
    F, A = hd.obs_features, hd.act_dim
    assert (F, A) == ((17, 4) if ik else (30, 7)) and hd.desc.rescale_actions == int(ik)
    W = torch.from_numpy(np.random.RandomState(4).uniform(-2, 2, (F, A)).astype(np.float32)).cuda()
    seen = []

    def policy(f):
        assert f.shape == (64, F) and f.dtype == torch.float32
        seen.append(f.clone())
        return torch.tanh((f.unsqueeze(2) * W.unsqueeze(0)).sum(dim=1))

    assert dev_env.collect_steps(policy, 9) is hd
    on_device, seen = seen, []
    low, high = host_env.action_space.low.astype(np.float64), host_env.action_space.high.astype(np.float64)
    obs = host_env.reset()
    for _ in range(9):
        f = np.concatenate([obs["achieved_goal"], obs["desired_goal"], obs["observation"]], axis=1)
        a = policy(torch.from_numpy(np.ascontiguousarray(f, np.float32)).cuda()).cpu().numpy()
        obs, _, _, _ = host_env.step(low + 0.5 * (a.astype(np.float64) + 1.0) * (high - low))   # SB3's unscale_action
    for k, (x, y) in enumerate(zip(on_device, seen)):
        assert torch.equal(x, y), f"the policy's input at step {k}"
    assert hd.counts_host() == hh.counts_host() and hd.counts_host()[1] >= 64 * 8
    np.testing.assert_array_equal(hd.counts.cpu().numpy(), hh.counts.cpu().numpy())
    for e in range(64):
        x, y = hd.export(e), hh.export(e)
        assert x["w"] == 9 and set(x) == set(y)
        for key in x:
            np.testing.assert_array_equal(x[key], y[key], err_msg=f"env {e}: {key}")
    stats = hd.episode_stats_per_env(clear=False)
    np.testing.assert_array_equal(stats, hh.episode_stats_per_env(clear=False))
    assert np.all(stats[:, 0] >= 2) and dev_env.her.episode_stats()["episodes"] == int(stats[:, 0].sum())
    if ik:   # the stored actions are the agent's rows at the policy's scale, not the joint action the step left
        np.testing.assert_allclose(hd.export(0)["action"][:9], np.stack([policy(f)[0].cpu().numpy() for f in on_device]), rtol=0, atol=2e-7)
    with pytest.raises(RuntimeError, match="collect_steps"):
        dev_env.step_async(np.zeros((64, A)))
    dev_env.reset()
    dev_env.step(np.zeros((64, A)))
    dev_env.close()
    host_env.close()


def test_which_env_takes_which_policy_and_buffer():
    clips = hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300)
    flat = hrg.HipVecEnv(4, env_kwargs=dict(ENV_KW), clips=clips)
    with pytest.raises(NotImplementedError, match="attach_replay.*attach_her"):
        flat.attach_sac(batch_size=32)
    flat.attach_replay(64)
    with pytest.raises(NotImplementedError, match="MultiInputPolicy"):
        flat.attach_sac(batch_size=32, policy="MultiInputPolicy")
    assert flat.attach_sac(batch_size=32, policy="MlpPolicy").obs_dim == flat.replay.obs_dim
    flat.close()
    env = _goal_env(n=4)
    with pytest.raises(NotImplementedError, match="attach_replay.*attach_her"):
        env.attach_sac(batch_size=32)
    with pytest.raises(NotImplementedError, match="attach_her"):
        env.collect_steps(lambda f: f, 1)
    hb = env.attach_her(40)
    with pytest.raises(NotImplementedError, match="MlpPolicy"):
        env.attach_sac(batch_size=32, policy="MlpPolicy")
    assert env.sac is None
    learner = env.attach_sac(batch_size=32, policy="MultiInputPolicy")
    assert env.sac is learner and (learner.obs_dim, learner.act_dim) == (hb.obs_features, hb.act_dim) == (30, 7)
    env.close()
    # the goal wrapper's default keys (obs_keys=None: object-state, robot0_proprio-state, desired_goal) make a row of 6 + 6 + 33 values, which fits
    default = hrg.HipVecEnv(4, goal_env=True, env_kwargs=dict(ENV_KW), clips=clips)
    default.attach_her(40)
    assert default.attach_sac(batch_size=32).obs_dim == default.her.obs_features == 45
    default.close()
    # 57 observation columns fit the buffer's lanes, the feature row of 6 + 6 + 57 does not: refused before a learner exists, by the name of the remedy
    wide = _goal_env(n=4, obs_keys=["object-state", "goal_difference", "robot0_proprio-state", "desired_goal", "goal-state", "robot0_joint_pos"])
    hb = wide.attach_her(40)
    assert (hb.obs_dim, hb.obs_features) == (57, 69)
    with pytest.raises(NotImplementedError, match="obs_keys"):
        wide.attach_sac(batch_size=32)
    assert wide.sac is None
    with pytest.raises(NotImplementedError, match="obs_keys"):
        hb.observation()
    with pytest.raises(NotImplementedError, match="obs_keys"):
        hb.sample_features(4)
    import ctypes
    import torch
    from human_robot_gym_amd._lib import load_library
    out = torch.zeros(4, 69, device="cuda")
    assert load_library().hrg_her_features(hb.h, None, 4, ctypes.c_void_p(out.data_ptr()), None) == CONST["HRG_ERR_INVALID"]
    wide.close()


def test_abi_refusals_of_the_feature_sampler():
    import ctypes
    import torch
    from human_robot_gym_amd._lib import load_library
    buf, _ = _filled("reach")
    lib, vp = load_library(), ctypes.c_void_p
    cum = torch.zeros(5, dtype=torch.int64, device="cuda")
    torch.cumsum(buf.counts, 0, out=cum[1:])
    outs = [torch.empty(4, w, device="cuda") for w in (45, 45, 7, 1, 1)]
    ptr = lambda ts: [None if t is None else vp(t.data_ptr()) for t in ts]   # noqa: E731
    bad = CONST["HRG_ERR_INVALID"]
    assert lib.hrg_her_sample_features(buf.h, 0, vp(cum.data_ptr()), *ptr(outs), None, None) == bad
    assert lib.hrg_her_sample_features(buf.h, -3, vp(cum.data_ptr()), *ptr(outs), None, None) == bad
    for k in range(5):
        assert lib.hrg_her_sample_features(buf.h, 4, vp(cum.data_ptr()), *ptr(outs[:k] + [None] + outs[k + 1:]), None, None) == bad, k
    assert lib.hrg_her_sample_features(buf.h, 4, None, *ptr(outs), None, None) == bad
    assert lib.hrg_her_features(buf.h, None, 4, None, None) == bad
    assert lib.hrg_her_features(buf.h, vp(outs[0].data_ptr()), 0, vp(outs[1].data_ptr()), None) == bad
    assert lib.hrg_her_stats(buf.h, None, 0) == bad
    assert buf.counts_host()[2] == 0   # a refused call draws nothing
    assert lib.hrg_her_sample_features(buf.h, 4, vp(cum.data_ptr()), *ptr(outs), None, None) == 0 and buf.counts_host()[2] == 1
    # an empty buffer: the call is accepted and leaves its outputs as they were (the caller's check: size(), once per train call)
    empty = _buffer(4, 16, 6)
    marked = [torch.full((4, w), 7.0, device="cuda") for w in (45, 45, 7, 1, 1)]
    assert empty.size() == 0
    no_counts = torch.zeros(5, dtype=torch.int64, device="cuda")
    assert lib.hrg_her_sample_features(empty.h, 4, vp(no_counts.data_ptr()), *ptr(marked), None, None) == 0
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in marked)
    with pytest.raises(ValueError, match="no finished episode"):
        empty.require_samples()
    empty.close()
    buf.close()


def _trained(seed_steps=6):
    import torch
    env = _goal_env()
    hb = env.attach_her(40)
    learner = env.attach_sac(batch_size=32, learning_rate=5e-4, ent_coef="auto_0.2")
    assert learner.desc.seed == 11
    with pytest.raises(ValueError, match="no finished episode"):
        learner.train(hb, 1)
    before = {k: v.clone() for k, v in learner.state_dict().items()}
    assert env.collect_steps(learner.act, seed_steps) is hb and hb.size() >= 64 * 4
    learner.train(hb, 4)
    torch.cuda.synchronize()
    return env, learner, before


def test_the_learner_trains_on_the_hindsight_buffer():
    """collect_steps with the learner's actor, then train(env.her, 4): every group of parameters moves, the targets by less than the critics, everything stays
    finite; the sampler's call counter and n_updates advanced by 4.  Two identically seeded runs end bit-identical."""
    import torch
    env, learner, before = _trained()
    after = learner.state_dict()
    assert all(bool(torch.isfinite(v).all()) for v in after.values())
    moved = lambda prefix: max(float((after[k] - before[k]).abs().max()) for k in after if k.startswith(prefix))   # noqa: E731
    assert moved("actor.") > 0 and moved("critic.qf0.") > 0 and moved("critic.qf1.") > 0 and moved("log_ent_coef") > 0
    assert 0 < moved("critic_target.") < min(moved("critic.qf0."), moved("critic.qf1."))
    diag = learner.diagnostics()
    assert set(diag) == {"ent_coef", "actor_loss", "critic_loss", "ent_coef_loss", "n_updates"} and all(math.isfinite(v) for v in diag.values()) and diag["n_updates"] == 4
    assert env.her.counts_host()[2] == 4
    with pytest.raises(ValueError, match="the learner takes"):   # a buffer of another width
        other = _buffer(4, 16, 6)
        try:
            learner.train(other, 1)
        finally:
            other.close()
    env2, learner2, _ = _trained()
    assert torch.equal(learner.p.params, learner2.p.params) and torch.equal(learner.p.target, learner2.p.target)
    assert torch.equal(learner.p.adam_m, learner2.p.adam_m) and torch.equal(learner.p.adam_v, learner2.p.adam_v)
    env.close()
    env2.close()


def test_a_step_on_dict_samples_is_a_step_on_their_concatenation():
    import torch
    from human_robot_gym_amd.replay import ReplayBufferSamples
    from human_robot_gym_amd.sac import SacLearner
    buf, _ = _filled("cube")
    a, b = (SacLearner(buf.obs_features, buf.act_dim, batch_size=64, seed=3) for _ in range(2))
    for _ in range(3):
        d = buf.sample(64)
        a.step(d)
        b.step(ReplayBufferSamples(_cat(d.observations), d.actions, _cat(d.next_observations), d.dones, d.rewards))
    torch.cuda.synchronize()
    assert torch.equal(a.p.params, b.p.params) and torch.equal(a.p.target, b.p.target) and a.n_updates == b.n_updates == 3
    fresh = SacLearner(buf.obs_features, buf.act_dim, batch_size=64, seed=3)
    assert not torch.equal(a.p.params, fresh.p.params)
    fresh.close()
    a.close()
    b.close()
    buf.close()
