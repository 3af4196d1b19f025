"""Hindsight experience replay on the device (csrc/hrgym_her.h): the add / observe / sample / reward-done kernels against tests/her_ref.py on synthetic
device tensors, the ABI's refusals, and the buffer behind HipVecEnv's reset / step against what the host received.  -m gpu.

Sizes: rings of 8 and 16 slots with horizons 5 and 6 (whole episodes leave the ring every few steps), one ring of 150 slots with a 70-step episode (the
back-fill loop strides past the 64 lanes), sample batches of 1, 63, 64, 65 and 257 (four samples per 256-thread block: a block with one wave, full blocks,
a last block with one wave)."""
import ctypes

import numpy as np
import pytest

import her_ref as R
import human_robot_gym_amd as hrg
from human_robot_gym_amd._cstruct import CONST

pytestmark = pytest.mark.gpu

# the policy's view the goal-env wrapper builds by default (object-state, robot0_proprio-state, desired_goal) and where the goal sits in it
OBS_COLS = {"reach": list(range(0, 12)) + list(range(18, 33)) + list(range(33, 39)), "cube": list(range(0, 12)) + list(range(18, 33)) + list(range(50, 53))}
DG_IN_OBS = {"reach": list(range(27, 33)), "cube": list(range(27, 30))}
# thresholds in the middle of the distances of random rows, so that relabelled samples fall on both sides; every reward term differs from its default
PARAMS = {"reach": dict(goal_dist=1.9, task_reward=1.5, object_gripped_reward=-0.5, reward_shaping=1, collision_reward=-3.0, reward_scale=2.0, done_at_success=1, done_at_collision=1),
          "cube": dict(goal_dist=0.9, task_reward=1.5, object_gripped_reward=-0.5, reward_shaping=0, collision_reward=-3.0, reward_scale=2.0, done_at_success=1, done_at_collision=0)}
OUT_KEYS = ("observation", "achieved_goal", "desired_goal", "next_observation", "next_achieved_goal", "next_desired_goal")


def _buffer(n, cap, horizon, kind="reach", ratio=0.8, strategy="future", seed=11, act_dim=7, bounds=None, relabel_observation=False, obs_cols=None):
    from human_robot_gym_amd.her import HerBuffer, build_her_desc
    desc = build_her_desc(n, cap, horizon, kind, OBS_COLS[kind] if obs_cols is None else obs_cols, act_dim=act_dim, ratio=ratio, goal_selection_strategy=strategy, seed=seed,
                          act_low=None if bounds is None else bounds[0], act_high=None if bounds is None else bounds[1],
                          dg_in_obs=DG_IN_OBS[kind] if relabel_observation else (), relabel_observation=relabel_observation, **PARAMS[kind])
    return HerBuffer(desc)


def _dev(step):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in step]


def _mask(m):
    import torch
    return None if m is None else torch.from_numpy(np.asarray(m, np.uint8)).cuda()


def _assert_ring_equal(buf, ring, what):
    for e in range(ring.n):
        got, want = buf.export(e), ring.export(e)
        assert set(got) == set(want)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: env {e}: {k}")
    np.testing.assert_array_equal(buf.counts.cpu().numpy(), ring.counts(), err_msg=what)
    stored, closed, _ = buf.counts_host()
    assert (stored, closed) == (int((ring.w - ring.tail).sum()), int(ring.counts().sum())) and buf.size() == closed


@pytest.mark.parametrize("bounds", [None, ([-0.1, -0.1, -0.1, -1.0], [0.1, 0.1, 0.1, 1.0])], ids=["agent-rows", "rescaled"])
def test_add_and_masked_observe_fill_the_rings_like_the_reference(bounds):
    """3 envs, 8 slots, horizon 5, 40 steps: the rings wrap five times and whole episodes leave them; after every step the exported rings are bit-equal to
    her_ref's (rows, actions, flags, ep_start, ep_len, w, tail, open, cur_obs).  A masked observe in mid-episode discards that env's open episode only."""
    n, cap, horizon = 3, 8, 5
    act_dim = 7 if bounds is None else 4
    buf, ring = _buffer(n, cap, horizon, act_dim=act_dim, bounds=bounds), R.Ring(n, cap, act_dim=act_dim, act_bounds=bounds)
    first = np.random.RandomState(0).uniform(-1, 1, (n, 64)).astype(np.float32)
    buf.observe(_dev([first])[0])
    ring.observe(first)
    _assert_ring_equal(buf, ring, "after the first observe")
    dropped = discarded = 0
    for k, step in enumerate(R.scripted_steps(n, 40, horizon, seed=1)):
        tail0 = ring.tail.copy()
        buf.add_step(*_dev(step))
        ring.add(*step)
        dropped += int((ring.tail > tail0).sum())
        _assert_ring_equal(buf, ring, f"step {k}")
        if k in (9, 17, 30):
            mask = np.array([0, 1, 0], np.uint8) if k != 30 else np.array([1, 0, 1], np.uint8)
            discarded += int(((ring.w > ring.open) & (mask != 0)).sum())
            kept = ring.w[mask == 0].copy()
            obs = step[1] + np.float32(1)
            buf.observe(_dev([obs])[0], _mask(mask))
            ring.observe(obs, mask)
            assert np.all(ring.w[mask != 0] == ring.open[mask != 0]) and np.array_equal(ring.w[mask == 0], kept)
            _assert_ring_equal(buf, ring, f"masked observe after step {k}")
    assert dropped >= 8 and discarded >= 2 and np.all(ring.w >= 3 * cap)
    if bounds is not None:   # the rescaled actions were clipped on both sides
        assert (ring.action == 1).any() and (ring.action == -1).any() and (np.abs(ring.action) < 1).any()
    buf.close()


def test_back_fill_of_an_episode_longer_than_the_wavefront():
    """2 envs, 150 slots, one 70-step episode: ep_len is written over all 70 slots (the lanes stride by 64)."""
    n, cap, horizon = 2, 150, 70
    buf, ring = _buffer(n, cap, horizon), R.Ring(n, cap)
    zero = np.zeros((n, 64), np.float32)
    buf.observe(_dev([zero])[0])
    ring.observe(zero)
    for step in R.scripted_steps(n, 70, horizon, seed=4, p_done=0.0):
        buf.add_step(*_dev(step))
        ring.add(*step)
    assert np.all(ring.ep_len[:, :70] == 70) and np.all(ring.ep_len[:, 70:] == 0) and np.all(ring.open == 70)
    _assert_ring_equal(buf, ring, "after the 70-step episode")
    for step in R.scripted_steps(n, 3, horizon, seed=5, p_done=0.0):   # and the next episode starts behind it
        buf.add_step(*_dev(step))
        ring.add(*step)
    _assert_ring_equal(buf, ring, "three steps later")
    buf.close()


def _filled(kind, strategy="future", ratio=0.8, relabel_observation=False, seed=11):
    """4 envs, 16 slots, horizon 6, 45 steps; env 3 never closes an episode (it is reset before its time limit).  Returns (buffer, ring)."""
    n, cap, horizon = 4, 16, 6
    buf, ring = _buffer(n, cap, horizon, kind=kind, ratio=ratio, strategy=strategy, relabel_observation=relabel_observation, seed=seed), R.Ring(n, cap)
    zero = np.zeros((n, 64), np.float32)
    buf.observe(_dev([zero])[0])
    ring.observe(zero)
    for step in R.scripted_steps(n, 45, horizon, seed=2):
        step[4][3] = 0
        if ring.w[3] - ring.open[3] == horizon - 1:
            m = np.array([0, 0, 0, 1], np.uint8)
            buf.observe(_dev([step[1]])[0], _mask(m))
            ring.observe(step[1], m)
        buf.add_step(*_dev(step))
        ring.add(*step)
    assert ring.counts()[3] == 0 and np.all(ring.counts()[:3] > 0) and ring.w[3] > ring.open[3]
    return buf, ring


def _assert_sample_equal(buf, got, want, what):
    idx = buf.last_index.cpu().numpy()
    np.testing.assert_array_equal(idx, want["index"], err_msg=f"{what}: index")
    for k in OUT_KEYS + ("action",):
        g = (got.observations if k in OUT_KEYS[:3] else got.next_observations)[k.replace("next_", "")] if k in OUT_KEYS else got.actions
        np.testing.assert_array_equal(g.cpu().numpy(), want[k], err_msg=f"{what}: {k}")
    np.testing.assert_array_equal(got.dones.cpu().numpy(), want["done"], err_msg=f"{what}: done")
    np.testing.assert_allclose(got.rewards.cpu().numpy(), want["reward"], rtol=1e-6, atol=1e-6, err_msg=f"{what}: reward")


@pytest.mark.parametrize("kind", ["reach", "cube"])
@pytest.mark.parametrize("strategy", ["future", "final", "episode"])
def test_samples_are_the_references(oracle_lib, kind, strategy):
    """Batches of 1, 63, 64, 65 and 257 at her_ratio 0, 0.8 and 1: transition, goal, gathered rows, actions and done flags bit-equal to her_ref, rewards
    at rtol 1e-6 / atol 1e-6 (FP64 with the device's approximate sqrt).  No compared sample sits within 1e-6 of the success threshold."""
    u01 = oracle_lib.hrgo_test_u01
    seam = gripped = success = failure = 0
    for ratio in (0.0, 0.8, 1.0):
        buf, ring = _filled(kind, strategy, ratio)
        buf.record_index = True
        for call, B in enumerate((1, 63, 64, 65, 257)):
            want = R.sample(ring, u01, 11, call, B, kind, ratio, strategy, params=PARAMS[kind], obs_cols=OBS_COLS[kind])
            assert want["margin"].min() >= 1e-6   # a threshold flip cannot hide in the reward tolerance
            assert buf.counts_host()[2] == call
            got = buf.sample(B)
            _assert_sample_equal(buf, got, want, f"{kind} {strategy} ratio {ratio} batch {B}")
            assert np.all(want["index"][:, 0] != 3)   # the env without a closed transition
            assert want["relabel"].all() if ratio == 1.0 else not want["relabel"].any() if ratio == 0.0 else B == 1 or 0 < want["relabel"].sum() < B
            e, i, g = want["index"].T
            rl = want["relabel"]
            seam += int((rl & (g % ring.cap < i % ring.cap)).sum()) + int((i % ring.cap == ring.cap - 1).sum())   # the goal's slot wrapped past the seam / the last slot
            near = rl & (R.goal_distance(kind, want["next_achieved_goal"], want["desired_goal"]) <= PARAMS[kind]["goal_dist"])   # relabelled into a success
            success += int(near.sum())
            failure += int((rl & ~near).sum())
            gripped += int((rl & ~near & (want["next_achieved_goal"][:, -1] != 0)).sum()) if kind == "cube" else 0
        assert buf.counts_host()[2] == 5
        buf.close()
    assert seam > 0 and success > 20 and failure > 20 and (kind == "reach" or gripped > 10)


def test_a_sample_does_not_depend_on_the_size_of_its_batch(oracle_lib):
    """The first 65 samples of a 257-sample call equal a 65-sample call made at the same call counter (two buffers filled alike)."""
    (a, ring), (b, _) = _filled("reach"), _filled("reach")
    a.record_index = b.record_index = True
    for buf in (a, b):
        buf.sample(7)   # both at call 1
    ga, gb = a.sample(257), b.sample(65)
    want = R.sample(ring, oracle_lib.hrgo_test_u01, 11, 1, 65, "reach", 0.8, params=PARAMS["reach"], obs_cols=OBS_COLS["reach"])
    _assert_sample_equal(b, gb, want, "65 at call 1")
    np.testing.assert_array_equal(a.last_index.cpu().numpy()[:65], b.last_index.cpu().numpy())
    for x, y in ((ga.actions, gb.actions), (ga.rewards, gb.rewards), (ga.dones, gb.dones)) + tuple((ga.observations[k], gb.observations[k]) for k in ga.observations) + tuple(
            (ga.next_observations[k], gb.next_observations[k]) for k in ga.next_observations):
        np.testing.assert_array_equal(x.cpu().numpy()[:65], y.cpu().numpy())
    a.close()
    b.close()


@pytest.mark.parametrize("kind", ["reach", "cube"])
def test_relabel_observation_rewrites_exactly_the_goal_columns(oracle_lib, kind):
    (on, ring), (off, _) = _filled(kind, relabel_observation=True), _filled(kind)
    on.record_index = off.record_index = True
    g1, g0 = on.sample(257), off.sample(257)
    want = R.sample(ring, oracle_lib.hrgo_test_u01, 11, 0, 257, kind, 0.8, params=PARAMS[kind], obs_cols=OBS_COLS[kind], relabel_observation=True, dg_in_obs=DG_IN_OBS[kind])
    _assert_sample_equal(on, g1, want, f"{kind} relabel_observation")
    np.testing.assert_array_equal(on.last_index.cpu().numpy(), off.last_index.cpu().numpy())
    rl, at = want["relabel"], DG_IN_OBS[kind]
    rest = [c for c in range(len(OBS_COLS[kind])) if c not in at]
    for key in ("observation",):
        for a, b in ((g1.observations[key], g0.observations[key]), (g1.next_observations[key], g0.next_observations[key])):
            a, b = a.cpu().numpy(), b.cpu().numpy()
            np.testing.assert_array_equal(a[:, rest], b[:, rest])                                  # nothing else changed
            np.testing.assert_array_equal(a[~rl], b[~rl])                                          # nor any sample that was not relabelled
            np.testing.assert_array_equal(a[rl][:, at], g1.observations["desired_goal"].cpu().numpy()[rl])   # the goal columns carry the new goal
            assert np.any(b[rl][:, at] != g0.observations["desired_goal"].cpu().numpy()[rl])       # which without the switch stay stale (the reference)
    for k in ("achieved_goal", "desired_goal"):
        np.testing.assert_array_equal(g1.observations[k].cpu().numpy(), g0.observations[k].cpu().numpy())
    on.close()
    off.close()


@pytest.mark.parametrize("env_id", ["ReachHuman", "PickPlaceHumanCart"])
def test_goal_reward_done_kernel_is_the_hosts_compute_reward_and_compute_done(env_id):
    """hrg_goal_reward_done on 64 random rows against HipVecEnv.compute_reward / compute_done of an env with every reward term set."""
    import torch
    kind = "reach" if env_id == "ReachHuman" else "cube"
    kw = dict({k: v for k, v in PARAMS[kind].items() if kind == "cube" or k != "object_gripped_reward"}, shield_type="OFF", horizon=12, seed=6, done_at_success=True,
              done_at_collision=True, reward_shaping=True)
    env = hrg.HipVecEnv(2, env_id=env_id, env_kwargs=kw, clips=hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300), goal_env=True)
    buf = env.attach_her(16)
    rng = np.random.RandomState(3)
    ag = rng.uniform(-1, 1, (64, len(R.AG_COLS[kind]))).astype(np.float32)
    if kind == "cube":
        ag[:, 6] = rng.randint(0, 2, 64)
    dg = rng.uniform(-1, 1, (64, len(R.DG_COLS[kind]))).astype(np.float32)
    ctype = rng.choice([0, 1, 2, 4, 8, 16], 64).astype(np.int32)
    infos = [dict(collision_type=int(c)) for c in ctype]
    dist = R.goal_distance(kind, ag, dg)
    assert np.abs(dist - kw["goal_dist"]).min() >= 1e-6 and 5 < (dist <= kw["goal_dist"]).sum() < 59
    want_r, want_d = env.compute_reward(ag, dg, infos), env.compute_done(ag, dg, infos)
    r, d = buf.compute_reward_done(torch.from_numpy(ag).cuda(), torch.from_numpy(dg).cuda(), torch.from_numpy(ctype).cuda())
    np.testing.assert_allclose(r.cpu().numpy(), want_r, rtol=1e-6, atol=1e-6)
    np.testing.assert_array_equal(d.cpu().numpy(), want_d)
    assert want_d.any() and not want_d.all() and len(set(np.round(want_r, 3))) > 20
    env.close()


def test_abi_refusals():
    import torch
    from human_robot_gym_amd._lib import HrgError, load_library
    from human_robot_gym_amd.her import HerBuffer, build_her_desc
    mk = lambda **k: build_her_desc(**dict(dict(n_envs=2, capacity=8, horizon=5, goal_kind="reach", obs_cols=range(64)), **k))   # noqa: E731
    for bad, code in ((dict(capacity=5), -1), (dict(capacity=4), -1), (dict(goal_kind=7), -4), (dict(obs_cols=[64]), -1), (dict(act_dim=8), -1)):
        with pytest.raises(HrgError, match=f"hrgym error {code}:"):
            HerBuffer(mk(**bad))
    d = mk()
    d.strategy = 3
    with pytest.raises(HrgError, match="hrgym error -4:"):
        HerBuffer(d)
    buf = HerBuffer(mk())
    with pytest.raises(HrgError, match="hrgym error -1:.*nothing to sample"):   # no closed transition yet
        buf.sample(4)
    for step in R.scripted_steps(2, 6, 5, seed=1):
        buf.add_step(*_dev(step))
    assert buf.size() > 0 and buf.sample(4).rewards.shape == (4, 1)
    lib, vp = load_library(), ctypes.c_void_p
    cum = torch.zeros(3, dtype=torch.int64, device="cuda")
    torch.cumsum(buf.counts, 0, out=cum[1:])
    outs = [torch.empty(4, w, device="cuda") for w in (64, 6, 6, 64, 6, 6, 7, 1, 1)]
    ptr = lambda ts: [None if t is None else vp(t.data_ptr()) for t in ts]   # noqa: E731
    assert lib.hrg_her_sample(buf.h, 0, vp(cum.data_ptr()), *ptr(outs), None, None) == CONST["HRG_ERR_INVALID"]
    assert lib.hrg_her_sample(buf.h, -3, vp(cum.data_ptr()), *ptr(outs), None, None) == CONST["HRG_ERR_INVALID"]
    for k in range(9):
        assert lib.hrg_her_sample(buf.h, 4, vp(cum.data_ptr()), *ptr(outs[:k] + [None] + outs[k + 1:]), None, None) == CONST["HRG_ERR_INVALID"], k
    assert lib.hrg_her_sample(buf.h, 4, None, *ptr(outs), None, None) == CONST["HRG_ERR_INVALID"]
    assert buf.counts_host()[2] == 1   # a refused call draws nothing
    assert lib.hrg_her_sample(buf.h, 4, vp(cum.data_ptr()), *ptr(outs), None, None) == 0 and buf.counts_host()[2] == 2
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="expected a contiguous"):
        buf.add_step(*[x[:1] for x in _dev(step)])
    buf.close()


def _rescaled(a, space):
    """custom_add 64-76: 2 (a - low) / (high - low) - 1 in FP64 over the space's f32 bounds, clipped, as f32."""
    low, high = space.low.astype(np.float64), space.high.astype(np.float64)
    return np.clip(2.0 * ((np.asarray(a, np.float64) - low) / (high - low)) - 1.0, -1, 1).astype(np.float32)


@pytest.mark.parametrize("front_end", ["ik", "collision_prevention"])
def test_stored_actions_behind_an_action_front_end_are_at_the_policys_scale(front_end):
    """Behind the IK front-end (PickPlaceHumanCart, [dx, dy, dz, gripper] within +-0.15) the buffer keeps the AGENT's row -- the step rewrites it into a
    joint action -- rescaled to [-1, 1] by the action bounds and clipped; under collision prevention (ReachHuman) it keeps the EXECUTED row,
    infos["action"], rescaled alike (HER_buffer_add_monkey_patch.py:64-79).  4 envs, horizon 6, 10 steps, some values outside the bounds."""
    clips = hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300)
    kw = dict(shield_type="OFF", horizon=6, seed=3)
    if front_end == "ik":
        env = hrg.HipVecEnv(4, env_id="PickPlaceHumanCart", env_kwargs=kw, clips=clips, goal_env=True, ik_position_delta=dict(action_limit=0.15))
    else:
        env = hrg.HipVecEnv(4, env_kwargs=kw, clips=clips, goal_env=True, collision_prevention=dict(replace_type=0, n_resamples=20))
    space = env.action_space
    width = space.shape[0]
    assert width == (4 if front_end == "ik" else 7)
    buf = env.attach_her(16)
    assert (buf.act_dim, buf.desc.rescale_actions) == (width, 1)
    np.testing.assert_array_equal(np.array(buf.desc.act_high[:width]), space.high.astype(np.float64))
    np.testing.assert_array_equal(np.array(buf.desc.act_low[:width]), space.low.astype(np.float64))
    env.reset()
    rng = np.random.RandomState(1)
    sent, executed = [], []
    for k in range(10):
        a = rng.uniform(1.25 * space.low.astype(np.float64), 1.25 * space.high.astype(np.float64), (4, width))
        if front_end != "ik":
            a[k % 4] = [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]   # the shoulder folding down: sooner or later into the table, which the screening replaces
        _, _, _, infos = env.step(a)
        sent.append(a)
        executed.append(np.stack([i["action"] for i in infos]))
    sent, executed = np.array(sent), np.array(executed)
    if front_end == "ik":
        assert executed.shape == (10, 4, 7) and not np.array_equal(executed[:, :, :4], sent)   # the step did rewrite the rows (joint actions)
        want = _rescaled(sent, space)
    else:
        want = _rescaled(executed, space)
    assert (want == 1).any() and (want == -1).any() and (np.abs(want) < 1).any()
    for e in range(4):
        x = buf.export(e)
        assert (x["w"], x["tail"]) == (10, 0)
        np.testing.assert_array_equal(x["action"][:10], want[:, e], err_msg=f"env {e}")
    s = buf.sample(64)
    assert s.actions.shape == (64, width) and float(s.actions.abs().max()) <= 1.0
    env.close()


def _training_config(n_sampled_goal):
    from types import SimpleNamespace as NS
    return NS(robot=NS(name="Schunk"), wrappers=NS(),
              environment=NS(env_id="ReachHuman", horizon=12, shield_type="OFF", reward_shaping=False, goal_dist=0.05, seed=5),
              run=NS(n_envs=4, seed=5, env_type="goal_env", obs_keys=None, expert_obs_keys=None, start_index=0, monitor_dir=None, monitor_kwargs=None,
                     vec_env_kwargs=dict(clips=hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300))),
              algorithm=NS(buffer_size=128, replay_buffer_kwargs=NS(n_sampled_goal=n_sampled_goal, goal_selection_strategy="future", online_sampling=True)))


def test_the_buffer_behind_reset_and_step_holds_what_the_host_received(oracle_lib):
    """create_training_vec_env with algorithm.replay_buffer_kwargs (4 ReachHuman goal envs, horizon 12, 32 slots each), 30 random steps: every stored
    transition is what reset / step returned -- dict observations, terminal_observation, reward, done, TimeLimit.truncated, infos["action"].  With the
    sparse reward and goal_dist 0.05 only hindsight makes successes: 1024 samples at her_ratio 0.8 hold more of them than 1024 at her_ratio 0."""
    from human_robot_gym_amd.her import HerBuffer
    env = hrg.create_training_vec_env(_training_config(4))
    assert env.her is not None and env.her.capacity == 32 and env.her.desc.her_ratio == 0.8 and env.her.desc.seed == 5
    plain = HerBuffer(env._her_desc(4, 32, 0, "future", False, None))   # her_ratio 0, fed the same device tensors
    assert plain.desc.her_ratio == 0.0
    back = env._backend
    prev = env.reset()
    plain.observe(back.batch.obs)
    rng = np.random.RandomState(0)
    tape = []
    for k in range(30):
        act = rng.uniform(-1, 1, (4, 7))
        obs, rew, done, infos = env.step(act)
        plain.add_step(back._act, back.batch.obs, back.batch.term_obs, back.batch.reward, back.batch.done, back.batch.info)
        post = {key: np.stack([infos[i]["terminal_observation"][key] if done[i] else obs[key][i] for i in range(4)]) for key in obs}
        tape.append(dict(pre=prev, post=post, reward=rew, done=done, trunc=np.array([bool(i.get("TimeLimit.truncated", False)) for i in infos]),
                         action=np.stack([i["action"] for i in infos]), ctype=np.array([i["collision_type"] for i in infos])))
        np.testing.assert_array_equal(tape[-1]["action"], act)   # no action front-end: the agent's rows
        prev = obs
    n_done = sum(int(t["done"].sum()) for t in tape)
    assert n_done >= 8 and sum(int(t["trunc"].sum()) for t in tape) >= 8   # horizon 12: every env timed out twice
    ring = R.Ring(4, 32)
    for e in range(4):
        x = env.her.export(e)
        assert (x["w"], x["tail"]) == (30, 0) and x["open"] == 1 + max(k for k in range(30) if tape[k]["done"][e])
        for k, t in enumerate(tape):   # slot k holds step k
            for key, cols in (("observation", env._cols), ("achieved_goal", env._ag_cols), ("desired_goal", env._dg_cols)):
                np.testing.assert_array_equal(x["pre"][k][cols], t["pre"][key][e], err_msg=f"env {e} step {k} {key}")
                np.testing.assert_array_equal(x["post"][k][cols], t["post"][key][e], err_msg=f"env {e} step {k} next {key}")
            assert x["reward"][k] == t["reward"][e] and bool(x["done"][k]) == bool(t["done"][e]) and bool(x["truncated"][k]) == bool(t["trunc"][e])
            assert x["collision_type"][k] == t["ctype"][e]
            np.testing.assert_array_equal(x["action"][k], t["action"][e].astype(np.float32))
        np.testing.assert_array_equal(x["cur_obs"][env._cols], prev["observation"][e])
        y = plain.export(e)
        for key in x:
            np.testing.assert_array_equal(x[key], y[key], err_msg=key)
            if key not in ("w", "tail", "open"):
                getattr(ring, key)[e] = x[key]
        ring.w[e], ring.tail[e], ring.open[e] = x["w"], x["tail"], x["open"]
    p = {k: getattr(env._desc, k) for k in R.PARAMS}
    assert p["goal_dist"] == 0.05 and not p["reward_shaping"]
    success = p["task_reward"] * p["reward_scale"]
    ref = {ratio: R.sample(ring, oracle_lib.hrgo_test_u01, 5, 0, 1024, "reach", ratio, params=p, obs_cols=env._cols) for ratio in (0.8, 0.0)}
    n_ref = {ratio: int((s["reward"] == success).sum()) for ratio, s in ref.items()}
    assert n_ref[0.8] > n_ref[0.0] and n_ref[0.8] > 0 and min(s["margin"].min() for s in ref.values()) >= 1e-6
    env.her.record_index = plain.record_index = True
    got = {0.8: env.her.sample(1024), 0.0: plain.sample(1024)}
    n_got = {ratio: int((s.rewards.cpu().numpy() == np.float32(success)).sum()) for ratio, s in got.items()}
    print(f"[her] successes among 1024 samples: her_ratio 0.8 -> {n_got[0.8]}, 0 -> {n_got[0.0]} (her_ref: {n_ref[0.8]}, {n_ref[0.0]})")
    assert n_got[0.8] > n_got[0.0] and n_got == n_ref
    _assert_sample_equal(env.her, got[0.8], ref[0.8], "through the env, her_ratio 0.8")
    _assert_sample_equal(plain, got[0.0], ref[0.0], "her_ratio 0")
    assert got[0.8].observations["observation"].shape == (1024, 33) and got[0.8].actions.shape == (1024, 7)
    assert env.her.add(1, 2, x=3) is None and env.her.size() == int(ring.counts().sum())
    plain.close()
    env.close()
