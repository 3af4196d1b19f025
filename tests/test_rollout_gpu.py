"""The PPO rollout buffer on the device (csrc/hrgym_rollout.h): the view / observe / add / GAE / get kernels against tests/rollout_ref.py on synthetic device
tensors, bit for bit; the ABI's refusals; HipVecEnv.collect_rollout against the same policy driven through env.step on the host.  -m gpu.

Sizes: 70 envs (two 64-thread blocks of the per-env kernels, the last partial; 18 four-wave blocks of the per-row kernels, the last half full) and 5 slots for
add / observe / get, (n, T) = (1, 1), (70, 5), (130, 64) for GAE (one lane, a partial block, a serial loop as long as the PPO run's), observations of 1, 18
(the PPO layout) and 64 values, actions of 4 and 7."""
import ctypes

import numpy as np
import pytest

import rollout_ref as R
import human_robot_gym_amd as hrg
from human_robot_gym_amd._cstruct import CONST, RolloutDesc

pytestmark = pytest.mark.gpu

COLS = {1: [37], 18: list(range(18)), 64: [int(c) for c in np.random.RandomState(5).permutation(64)]}
F32_KEYS = ("observations", "actions", "rewards", "values", "log_probs", "episode_starts", "advantages", "returns", "cur_obs", "flags")


def _buffer(n, T, K=18, act_dim=7, gamma=0.99, gae_lambda=0.9, seed=0):
    from human_robot_gym_amd.rollout import RolloutBuffer, build_rollout_desc
    return RolloutBuffer(build_rollout_desc(n, T, COLS[K], act_dim=act_dim, gamma=gamma, gae_lambda=gae_lambda), seed=seed)


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _add(buf, ref, step, with_tv=True):
    a, v, lp, tv, obs, rew, dn, info = step
    tv = tv if with_tv else None
    buf.add_step(_dev(a), _dev(v), _dev(lp), _dev(tv), _dev(obs), None, _dev(rew), _dev(dn), _dev(info))
    ref.add(a, v, lp, tv, obs, rew, dn, info)


def _assert_bits_equal(got, want, what):
    """Every array of export(), bit for bit (float32 as uint32, float64 as uint64 views)."""
    assert set(got) == set(want)
    for k in want:
        g, w = got[k], want[k]
        if isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
            bits = {4: np.uint32, 8: np.uint64}[w.dtype.itemsize]
            np.testing.assert_array_equal(g.view(bits), w.view(bits), err_msg=f"{what}: {k}")
        else:
            assert g == w, (what, k, g, w)


def _done_pattern(n, T, seed):
    """Random (p = 0.3), with: env 0 done on the first step, env 1 on the last, env 2 on two consecutive steps, env 5 on every step, env 6 never."""
    d = (np.random.RandomState(seed).uniform(size=(T, n)) < 0.3).astype(np.uint8)
    if n > 6:
        d[:, :7] = 0
        d[0, 0] = d[T - 1, 1] = 1
        d[T // 2 - 1:T // 2 + 1, 2] = 1
        d[:, 5] = 1
    return d


@pytest.mark.parametrize("act_dim", [4, 7])
@pytest.mark.parametrize("K", [1, 18, 64])
def test_add_and_masked_observe_fill_the_buffer_like_the_reference(K, act_dim):
    """70 envs, 5 slots, two rollouts; terminal values given and NULL; after every call the whole export (slots, current rows, flags, running returns,
    episode accumulators) is bit-equal to rollout_ref's.  Step 3 truncates env 3 and terminates env 4; a masked observe follows step 2."""
    n, T = 70, 5
    for with_tv in (True, False):
        buf, ref = _buffer(n, T, K, act_dim, gamma=0.97), R.Rollout(n, T, COLS[K], act_dim, gamma=0.97, gae_lambda=0.9)
        first = np.random.RandomState(0).uniform(-1, 1, (n, 64)).astype(np.float32)
        buf.observe(_dev(first))
        ref.observe(first)
        _assert_bits_equal(buf.export(), ref.export(), "after the first observe")
        booted = 0
        for rollout in range(2):
            steps = list(R.scripted_steps(n, T, act_dim, seed=10 + rollout, done=_done_pattern(n, T, rollout)))
            dn, info = steps[3][6], steps[3][7]
            dn[3] = dn[4] = 1
            info[3, R.INFO_TRUNCATED], info[4, R.INFO_TRUNCATED] = 1, 0
            for k, step in enumerate(steps):
                before = ref.rewards.copy()
                _add(buf, ref, step, with_tv)
                booted += int((ref.rewards[k] != step[5]).sum())
                _assert_bits_equal(buf.export(), ref.export(), f"tv {with_tv} rollout {rollout} step {k}")
                assert np.array_equal(before[:k], ref.rewards[:k])
                if k == 2:
                    mask = (np.arange(n) % 3 == rollout).astype(np.uint8)
                    rows = step[4] + np.float32(1)
                    buf.observe(_dev(rows), _dev(mask))
                    ref.observe(rows, mask)
                    _assert_bits_equal(buf.export(), ref.export(), f"masked observe in rollout {rollout}")
            assert buf.full and buf.export()["pos"] == T
            last = np.random.RandomState(3).uniform(-1, 1, n).astype(np.float32)
            buf.compute_returns_and_advantage(_dev(last))
            ref.compute(last)
            _assert_bits_equal(buf.export(), ref.export(), f"computed, rollout {rollout}")
            buf.reset()
            ref.reset()
            _assert_bits_equal(buf.export(), ref.export(), f"reset after rollout {rollout}")
        assert (booted > 5) if with_tv else booted == 0
        assert ref.stats[5, 0] == 2 * T and ref.stats[6, 0] == 0 and ref.stats[:, 0].sum() > 100 and ref.run_length[6] == 7   # (env 6: observed again after step 2 of rollout 0)
        st = buf.episode_stats(clear=False)
        tot = ref.stats.sum(axis=0)
        assert (st["episodes"], st["r"], st["l"]) == (int(tot[0]), float(tot[1]), int(tot[2])) and st["n_goal_reached"] == tot[3 + 9] and len(st) == 3 + 14
        assert buf.episode_stats() == st and buf.episode_stats()["episodes"] == 0 and not buf.export()["stats"].any()   # cleared by the second call
        buf.close()


@pytest.mark.parametrize("n,T", [(1, 1), (70, 5), (130, 64)])
@pytest.mark.parametrize("gamma,lam", [(0.99, 0.9), (1.0, 1.0), (0.5, 0.0)])
def test_gae_is_the_float32_restatement_bit_for_bit(n, T, gamma, lam):
    buf, ref = _buffer(n, T, gamma=gamma, gae_lambda=lam), R.Rollout(n, T, COLS[18], gamma=gamma, gae_lambda=lam)
    zero = np.zeros((n, 64), np.float32)
    buf.observe(_dev(zero))
    ref.observe(zero)
    done = _done_pattern(n, T, seed=T)
    for step in R.scripted_steps(n, T, 7, seed=n, done=done):
        _add(buf, ref, step)
    if n > 6:
        assert done[:, 5].all() and not done[:, 6].any()
    last = np.random.RandomState(1).uniform(-1, 1, n).astype(np.float32)
    buf.compute_returns_and_advantage(_dev(last))
    ref.compute(last)
    got, want = buf.export(), ref.export()
    for k in ("advantages", "returns"):
        np.testing.assert_array_equal(got[k].view(np.uint32), want[k].view(np.uint32), err_msg=k)
    assert got["computed"] and np.isfinite(got["advantages"]).all()
    if (n, T, lam) == (130, 64, 0.9):   # the comparison would have caught a contracted recursion
        assert (R.gae_with_fma(ref, last).view(np.uint32) != ref.advantages.view(np.uint32)).mean() > 0.05
    buf.close()


@pytest.mark.parametrize("K", [1, 18, 64])
def test_view_is_the_column_selection(K):
    buf = _buffer(70, 5, K)
    for m in (1, 70, 259):   # one wave of one block; a half-full last block; more rows than envs, a last block with three waves
        rows = np.random.RandomState(m).uniform(-1, 1, (m, 64)).astype(np.float32)
        got = buf.view(_dev(rows))
        assert tuple(got.shape) == (m, K)
        np.testing.assert_array_equal(got.cpu().numpy(), rows[:, COLS[K]])
    rows = np.random.RandomState(9).uniform(-1, 1, (70, 64)).astype(np.float32)
    buf.observe(_dev(rows))
    np.testing.assert_array_equal(buf.observation().cpu().numpy(), rows[:, COLS[K]])
    with pytest.raises(ValueError, match="expected a contiguous"):
        buf.view(_dev(rows[:, :63]))
    buf.close()


def _computed(n=70, T=5, K=18, act_dim=7, seed=0):
    buf, ref = _buffer(n, T, K, act_dim, seed=seed), R.Rollout(n, T, COLS[K], act_dim, gae_lambda=0.9)
    for step in R.scripted_steps(n, T, act_dim, seed=4):
        _add(buf, ref, step)
    last = np.random.RandomState(1).uniform(-1, 1, n).astype(np.float32)
    buf.compute_returns_and_advantage(_dev(last))
    ref.compute(last)
    return buf, ref


def _assert_batch_is(batch, flat, idx, what):
    for field, key in zip(batch._fields, ("observations", "actions", "values", "log_probs", "advantages", "returns")):
        np.testing.assert_array_equal(getattr(batch, field).cpu().numpy(), flat[key][idx], err_msg=f"{what}: {field}")


def test_get_covers_one_permutation_in_minibatches():
    """N = 350, batch_size 64: six batches, the last of 30; the epoch's indices are 0 .. 349 once each; every field is the flat export at those indices."""
    import torch
    buf, ref = _computed()
    flat = ref.export()
    _assert_bits_equal(buf.export(), flat, "the buffer the batches come from")
    epochs = []
    for epoch in range(2):
        batches = list(buf.get(batch_size=64))
        perm = buf.last_indices.cpu().numpy()
        assert [int(b.old_values.shape[0]) for b in batches] == [64] * 5 + [30]
        assert perm.dtype == np.int64 and np.array_equal(np.sort(perm), np.arange(350))
        for k, b in enumerate(batches):
            assert tuple(b.observations.shape) == (len(perm[64 * k:64 * k + 64]), 18) and tuple(b.actions.shape) == (b.observations.shape[0], 7)
            _assert_batch_is(b, flat, perm[64 * k:64 * k + 64], f"epoch {epoch} batch {k}")
        epochs.append(perm)
    assert not np.array_equal(epochs[0], epochs[1]) and not np.array_equal(epochs[0], np.arange(350))   # the buffer's generator moves on
    (whole,) = list(buf.get())   # batch_size None: everything in one batch
    _assert_batch_is(whole, flat, buf.last_indices.cpu().numpy(), "whole buffer")
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    list(buf.get(64, generator=g))
    a = buf.last_indices.cpu().numpy()
    g.manual_seed(7)
    list(buf.get(350, generator=g))
    np.testing.assert_array_equal(buf.last_indices.cpu().numpy(), a)   # the caller's generator decides the permutation
    other, _ = _computed(seed=0)
    list(other.get(64))
    np.testing.assert_array_equal(other.last_indices.cpu().numpy(), epochs[0])   # and the buffer's own seed does otherwise
    other.close()
    buf.close()


def test_get_with_the_callers_indices():
    import torch
    buf, ref = _computed()
    flat = ref.export()
    idx = np.array([349, 0, 0, 17, 349, 64, 65, 0], np.int64)   # repeats, both ends, across a wave's and a block's seam
    (b,) = list(buf.get(indices=_dev(idx)))
    _assert_batch_is(b, flat, idx, "caller's indices")
    buf.reset()   # a refused call must not launch: with the position at 0 a launch attempt would be refused by the ABI with another error
    for bad, exc in ((np.array([0, 350], np.int64), IndexError), (np.array([-1, 3], np.int64), IndexError), (np.array([1, 2], np.int32), ValueError),
                     (np.zeros(0, np.int64), ValueError), (np.zeros((2, 2), np.int64), ValueError)):
        with pytest.raises(exc, match="indices"):
            list(buf.get(indices=_dev(bad)))
    with pytest.raises(ValueError, match="indices"):
        list(buf.get(indices=torch.from_numpy(idx)))   # on the host
    with pytest.raises(ValueError, match="not both"):
        list(buf.get(batch_size=4, indices=_dev(idx)))
    buf.close()


def _raw_desc(**k):
    d = RolloutDesc()
    d.n_envs, d.n_steps, d.gamma, d.gae_lambda, d.act_dim, d.n_obs_cols = 2, 3, 0.99, 0.95, 7, 18
    for c in range(18):
        d.obs_cols[c] = c
    for name, v in k.items():
        if name == "col":
            d.obs_cols[v[0]] = v[1]
        else:
            setattr(d, name, v)
    return d


def test_abi_refusals():
    from human_robot_gym_amd._lib import HrgError, load_library
    from human_robot_gym_amd.rollout import RolloutBuffer
    INVALID = CONST["HRG_ERR_INVALID"]
    cases = [(dict(n_envs=0), "n_envs and n_steps"), (dict(n_steps=0), "n_envs and n_steps"), (dict(n_envs=-4), "n_envs and n_steps"),
             (dict(n_obs_cols=0), "n_obs_cols"), (dict(n_obs_cols=65), "n_obs_cols"), (dict(col=(17, 64)), "column outside"), (dict(col=(0, -1)), "column outside"),
             (dict(act_dim=0), "act_dim"), (dict(act_dim=8), "act_dim"), (dict(gamma=-0.01), "gamma must lie"), (dict(gamma=1.01), "gamma must lie"),
             (dict(gae_lambda=-0.01), "gae_lambda must lie"), (dict(gae_lambda=1.01), "gae_lambda must lie"), (dict(gamma=float("nan")), "gamma must lie")]
    for bad, text in cases:
        with pytest.raises(HrgError, match=f"hrgym error {INVALID}: rollout: .*{text}"):
            RolloutBuffer(_raw_desc(**bad))
    assert _raw_desc(col=(18, 99)).obs_cols[18] == 99
    RolloutBuffer(_raw_desc(col=(18, 99))).close()   # behind n_obs_cols: not a column
    n, T = 2, 3
    buf = RolloutBuffer(_raw_desc())
    steps = list(R.scripted_steps(n, T + 1, 7, seed=1))
    dev = lambda s: (_dev(s[0]), _dev(s[1]), _dev(s[2]), _dev(s[3]), _dev(s[4]), None, _dev(s[5]), _dev(s[6]), _dev(s[7]))   # noqa: E731
    last = _dev(np.zeros(n, np.float32))
    idx = _dev(np.array([0, 5], np.int64))
    with pytest.raises(HrgError, match="not full yet"):
        buf.compute_returns_and_advantage(last)
    for s in steps[:T - 1]:
        buf.add_step(*dev(s))
    with pytest.raises(HrgError, match=f"hrgym error {INVALID}: rollout: the buffer is not full yet"):
        buf.compute_returns_and_advantage(last)
    buf.add_step(*dev(steps[T - 1]))
    with pytest.raises(HrgError, match=f"hrgym error {INVALID}: rollout: no returns and advantages yet"):
        list(buf.get(indices=idx))
    with pytest.raises(HrgError, match=f"hrgym error {INVALID}: rollout: the buffer is full"):
        buf.add_step(*dev(steps[T]))
    assert buf.export()["pos"] == T
    buf.compute_returns_and_advantage(last)
    assert len(list(buf.get(4))) == 2
    lib, vp = load_library(), ctypes.c_void_p
    outs = [_dev(np.zeros(s, np.float32)) for s in ((2, 18), (2, 7), (2,), (2,), (2,), (2,))]
    ptr = lambda ts: [None if t is None else vp(t.data_ptr()) for t in ts]   # noqa: E731
    assert lib.hrg_rollout_get(buf.h, vp(idx.data_ptr()), 0, *ptr(outs), None) == INVALID and b"batch_size" in lib.hrg_last_error()
    for k in range(6):
        assert lib.hrg_rollout_get(buf.h, vp(idx.data_ptr()), 2, *ptr(outs[:k] + [None] + outs[k + 1:]), None) == INVALID, k
    assert lib.hrg_rollout_get(buf.h, None, 2, *ptr(outs), None) == INVALID
    assert lib.hrg_rollout_get(buf.h, vp(idx.data_ptr()), 2, *ptr(outs), None) == 0
    buf.reset()   # a new rollout: the old advantages are not handed out
    with pytest.raises(HrgError, match="no returns and advantages yet"):
        list(buf.get(indices=idx))
    with pytest.raises(ValueError, match="expected a contiguous"):
        buf.add_step(*[None if x is None else x[:1] for x in dev(steps[0])])
    assert buf.pos == 0
    buf.close()


# ---- the device loop against the host loop --------------------------------------------------------------------------------------------------------
class _Policy:
    """A deterministic stand-in: fixed float32 linear maps and tanh, evaluated with torch on the device (products and a sum per output, row by row: a row's
    outputs do not depend on the other rows of its batch).  Actions reach 1.25 times the bounds, so some are clipped on their way into the env."""

    def __init__(self, K, space, seed=0):
        import torch
        rng = np.random.RandomState(seed)
        A = space.shape[0]
        self.Wa, self.wv = torch.from_numpy(rng.uniform(-1, 1, (K, A)).astype(np.float32)).cuda(), torch.from_numpy(rng.uniform(-1, 1, K).astype(np.float32)).cuda()
        self.scale = torch.from_numpy((1.25 * space.high).astype(np.float32)).cuda()
        self.torch = torch

    def value(self, obs):
        return self.torch.tanh((obs * self.wv).sum(1))

    def __call__(self, obs):
        a = self.torch.tanh((obs[:, :, None] * self.Wa[None]).sum(1)) * self.scale
        return a, self.value(obs), -(a * a).sum(1)


def _host_rollout(env, ref, pol, obs, tally):
    """collect_rollouts through env.step, as SB3 runs it: the policy on the uploaded observations, clipped actions into the env, the value of the terminal
    observation where truncated, into rollout_ref.  `tally`: per-env sums over the infos of done steps.  Returns the last observations."""
    n, keys = env.num_envs, env._info_keys
    ref.reset()
    for _ in range(ref.T):
        a, v, lp = (x.cpu().numpy() for x in pol(_dev(obs)))
        obs, rew, done, infos = env.step(np.clip(a, env.action_space.low, env.action_space.high))
        term, info = obs.copy(), np.zeros((n, R.INFO_DIM), np.int32)
        for i in np.nonzero(done)[0]:
            term[i] = infos[i]["terminal_observation"]
            info[i] = [int(infos[i].get(k, False)) for k in keys]
            tally[i, 0] += 1
            tally[i, 1] += infos[i]["episode"]["r"]
            tally[i, 2] += infos[i]["episode"]["l"]
            tally[i, 3:] += info[i]
        tv = pol.value(_dev(term)).cpu().numpy()
        ref.add(a, v, lp, tv, env._last_full, rew, done.astype(np.uint8), info)
    ref.compute(pol.value(_dev(obs)).cpu().numpy())
    return obs


@pytest.mark.parametrize("case", ["reach", "reach-collision-prevention", "pick-place-ik"])
def test_collect_rollout_is_the_host_loop(case):
    """8 envs, horizon 3, n_steps 7, two rollouts in a row: every env is truncated twice inside a rollout, and the second rollout starts in mid-episode.
    The export is bit-equal to rollout_ref fed by the host loop, episode_stats() equals the sums over the host loop's infos."""
    n, T = 8, 7
    clips = hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300)
    kw = dict(env_kwargs=dict(horizon=3, seed=11), clips=clips)
    if case == "pick-place-ik":
        kw.update(env_id="PickPlaceHumanCart", ik_position_delta=dict(action_limit=0.15))
    elif case == "reach-collision-prevention":
        kw.update(collision_prevention=dict(replace_type=0, n_resamples=20))
    dev_env, host_env = hrg.HipVecEnv(n, **kw), hrg.HipVecEnv(n, **kw)
    A = 4 if case == "pick-place-ik" else 7
    rb = dev_env.attach_rollout(T, gamma=0.99, gae_lambda=0.9)
    assert dev_env.rollout is rb and host_env.rollout is None and (rb.n, rb.n_steps, rb.act_dim, rb.obs_dim) == (n, T, A, len(dev_env._cols))
    pol = _Policy(rb.obs_dim, dev_env.action_space)
    ref = R.Rollout(n, T, dev_env._cols, A, gamma=0.99, gae_lambda=0.9)
    obs = host_env.reset()
    ref.observe(host_env._last_full)
    tally = np.zeros((n, R.STATS_DIM))
    for rollout in range(2):
        assert dev_env.collect_rollout(pol, pol.value) is rb
        obs = _host_rollout(host_env, ref, pol, obs, tally)
        want = ref.export()
        _assert_bits_equal(rb.export(), want, f"{case} rollout {rollout}")
        trunc = (want["episode_starts"].reshape(n, T)[:, 1:] != 0).sum(axis=1) + (want["flags"] != 0)
        assert np.all(trunc >= 2) and np.isfinite(want["advantages"]).all()
        assert (np.abs(want["actions"]) > np.abs(dev_env.action_space.high)).any()   # stored as the policy emitted them
    np.testing.assert_array_equal(rb.export()["stats"], tally)
    st, tot = rb.episode_stats(), tally.sum(axis=0)
    assert st["episodes"] == int(tot[0]) >= 4 * n and st["r"] == float(tot[1]) and st["l"] == int(tot[2]) and st["r"] != 0
    assert list(st)[3:] == dev_env._info_keys and [st[k] for k in dev_env._info_keys] == [float(x) for x in tot[3:]] and st["TimeLimit.truncated"] > 0
    # the device loop left the host accounting behind
    with pytest.raises(RuntimeError, match="step_async after collect_rollout"):
        dev_env.step_async(np.zeros((n, A)))
    first = dev_env.reset()
    np.testing.assert_array_equal(first, host_env.reset())
    o1, r1, d1, _ = dev_env.step(np.zeros((n, A)))
    o2, r2, d2, _ = host_env.step(np.zeros((n, A)))
    np.testing.assert_array_equal(o1, o2)
    np.testing.assert_array_equal(r1, r2)
    dev_env.close()
    host_env.close()


def test_collect_rollout_refusals_and_reseeding(tmp_path):
    clips = hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300)
    kw = dict(env_kwargs=dict(horizon=3, seed=11, shield_type="OFF"), clips=clips)
    env = hrg.HipVecEnv(2, monitor_dir=str(tmp_path), **kw)
    with pytest.raises(NotImplementedError, match="attach_rollout"):
        env.collect_rollout(None, None)
    rb = env.attach_rollout(4)
    assert (rb.gamma, rb.gae_lambda) == (0.99, 0.95)
    with pytest.raises(NotImplementedError, match="monitor_dir"):
        env.collect_rollout(None, None)
    env.seed(12)   # a rebuilt batch carries a new, empty buffer of the same shape
    assert env.rollout is not rb and (env.rollout.n_steps, env.rollout.gae_lambda) == (4, 0.95)
    env.close()
    for bad, text in ((dict(goal_env=True), "goal_env"), (dict(obs_norm=dict(mean=np.zeros(18), std=np.ones(18))), "obs_norm")):
        env = hrg.HipVecEnv(2, **kw, **bad)
        with pytest.raises(NotImplementedError, match=f"attach_rollout: {text}"):
            env.attach_rollout(4)
        env.close()
    env = hrg.HipVecEnv(2, expert=dict(id="ReachHuman"), imitation_reward=dict(alpha=0.5), **kw)
    with pytest.raises(NotImplementedError, match="attach_rollout: a dataset or an imitation reward"):
        env.attach_rollout(4)
    env.close()
    mixed = hrg.make_mixed_vec_env(2, tasks=hrg.ICRA_TASKS[:2], n_clips=3)
    with pytest.raises(NotImplementedError, match="attach_rollout: the mixed batch"):
        mixed.attach_rollout(4)
    mixed.close()


def _training_config(algorithm):
    from types import SimpleNamespace as NS
    return NS(robot=NS(name="Schunk"), wrappers=NS(), environment=NS(env_id="ReachHuman", horizon=12, shield_type="OFF", seed=5),
              run=NS(n_envs=4, seed=5, env_type="env", obs_keys=None, expert_obs_keys=None, start_index=0, monitor_dir=None, monitor_kwargs=None,
                     vec_env_kwargs=dict(clips=hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300))), algorithm=algorithm)


def test_the_config_path_attaches_the_buffer_for_ppo_only():
    from types import SimpleNamespace as NS
    env = hrg.create_training_vec_env(_training_config(NS(name="PPO", n_steps=16, gamma=0.98, gae_lambda=0.9, batch_size=64)))
    rb = env.rollout
    assert rb is not None and (rb.n, rb.n_steps, rb.gamma, rb.gae_lambda, rb.act_dim, rb.obs_dim) == (4, 16, 0.98, 0.9, 7, 18)
    assert list(rb.desc.obs_cols[:18]) == list(range(18))
    env.close()
    env = hrg.create_training_vec_env(_training_config(NS(name="SAC", gamma=0.99, buffer_size=1000)))
    assert env.rollout is None
    env.close()
