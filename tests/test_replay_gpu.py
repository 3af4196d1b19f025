"""The uniform replay buffer on the device (csrc/hrgym_replay.h): the view / observe / add / sample kernels against tests/replay_ref.py on synthetic device
tensors; the ABI's refusals; HipVecEnv.collect_steps against the same policy driven through env.step on the host, with the wrappers of the ICRA runs on.  -m gpu.

What is copied is compared bit for bit (actions, rewards, dones, timeouts, the position, the accumulators, observations without normalisation).  Normalised
observations: the device divides in double by reciprocal refinement (-fapprox-func) and its tanh is ocml's, each within a few float64 ulps of numpy's, so the
float32 result may differ from the restatement's only where the exact value sits within about 2^-50 relative of a float32 rounding boundary: every value within
ONE float32 ulp, and FEWER THAN 1 IN 1000 values different at all (the expected count is far below one; float32 arithmetic would differ in a large share of
the values: tests/test_replay.py).

Sizes: 70 envs (70 one-wavefront blocks of the per-env kernels; 18 four-wave blocks of the per-row kernels, the last half full), 5 slots and
12 adds (the ring wraps twice), (n, capacity) = (1, 1), observations of 1, 18 and 63 + time values, actions of 4 and 7, batches of 1 and 257."""
import ctypes

import numpy as np
import pytest

import replay_ref as R
import human_robot_gym_amd as hrg
from human_robot_gym_amd._cstruct import CONST, ReplayDesc

pytestmark = pytest.mark.gpu

COLS = {1: [37], 18: list(range(18)), 64: [int(c) for c in np.random.RandomState(5).permutation(64)[:63]]}   # 64: 63 columns + the time value
NORM = {1: None, 18: 0.5, 64: False}   # per layout: no normalisation; normalised and squashed; normalised
OBS_KEYS = ("observations", "next_observations")


def _stats(K, seed=0):
    """(mean, std, squash_factor) of layout K, std drawn from [0.1, 10]; Nones without normalisation."""
    if NORM[K] is None:
        return None, None, None
    rng = np.random.RandomState(seed)
    return rng.uniform(-1, 1, K), rng.uniform(0.1, 10, K), (NORM[K] or None)


def _pair(n, buffer_size, K=18, act_dim=7, seed=11):
    from human_robot_gym_amd.replay import ReplayBuffer, build_replay_desc
    mean, std, sf = _stats(K)
    buf = ReplayBuffer(build_replay_desc(n, buffer_size, COLS[K], act_dim=act_dim, observe_time=K == 64, mean=mean, std=std, squash_factor=sf, seed=seed))
    return buf, R.Replay(n, buffer_size, COLS[K], act_dim, observe_time=K == 64, mean=mean, std=std, squash_factor=sf)


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _rows(K, imit, sir):
    """Which imitation rows a layout's adds carry: the time column needs the state imitation rows; the 18-value layout takes the action-based ones."""
    return dict(sir=sir) if K == 64 else dict(imit=imit) if K == 18 else {}


def _add(buf, ref, step, K):
    a, obs, term, rew, dn, info, imit, sir = step
    rows = _rows(K, imit, sir)
    buf.add_step(_dev(a), _dev(obs), _dev(term), _dev(rew), _dev(dn), _dev(info), **{k: _dev(v) for k, v in rows.items()})
    ref.add(a, obs, term, rew, dn, info, **rows)


def _assert_normalised_close(got, want, what):
    """The tolerance of normalised observations (module docstring): within one float32 ulp, fewer than 1 in 1000 different.  Prints the figures first."""
    d = R.ulp_distance(got, want)
    print(f"[replay] {what}: {int((d != 0).sum())} of {d.size} normalised values differ, by at most {int(d.max()) if d.size else 0} ulp")
    assert np.isfinite(got).all() and d.max() <= 1, what
    assert (d != 0).sum() * 1000 < d.size, what


def _assert_export(got, want, normalised, what):
    """Every array of export(): bit for bit (float32 as uint32, float64 as uint64 views), but the normalised observations, which follow the tolerance."""
    assert set(got) == set(want)
    for k in want:
        g, w = got[k], want[k]
        if isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
            if normalised and k in OBS_KEYS:
                _assert_normalised_close(g, w, f"{what}: {k}")
                continue
            bits = {1: np.uint8, 4: np.uint32, 8: np.uint64}[w.dtype.itemsize]
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
def test_add_and_masked_observe_fill_the_ring_like_the_reference(K, act_dim):
    """70 envs, 5 slots, 12 adds: the ring wraps twice; after every call the whole export (slots, current rows and time values, running returns, episode
    accumulators, position) matches replay_ref's.  Step 3 truncates env 3 and terminates env 4; a masked observe follows step 2.  K = 1: plain columns, no
    imitation rows; K = 18: normalised and squashed, the action-based imitation rows; K = 64: 63 columns + the time column, normalised, the state rows."""
    n, cap, T = 70, 5, 12
    buf, ref = _pair(n, n * cap + 3, K, act_dim)
    assert (buf.capacity, buf.obs_dim, buf.act_dim, buf.size()) == (cap, K, act_dim, 0)
    norm = NORM[K] is not None
    rng = np.random.RandomState(0)
    first, t0 = rng.uniform(-1, 1, (n, 64)).astype(np.float32), rng.uniform(0, 1, n).astype(np.float32)
    time = dict(time=t0) if K == 64 else {}
    buf.observe(_dev(first), **{k: _dev(v) for k, v in time.items()})
    ref.observe(first, **time)
    _assert_export(buf.export(), ref.export(), norm, "after the first observe")
    np.testing.assert_array_equal(R.ulp_distance(buf.observation().cpu().numpy(), ref.last_view) > (1 if norm else 0), False)
    steps = list(R.scripted_steps(n, T, act_dim, seed=10, done=_done_pattern(n, T, 0)))
    dn, info = steps[3][4], steps[3][5]
    dn[3] = dn[4] = 1
    info[3, R.INFO_TRUNCATED], info[4, R.INFO_TRUNCATED] = 1, 0
    for k, step in enumerate(steps):
        _add(buf, ref, step, K)
        _assert_export(buf.export(), ref.export(), norm, f"K {K} step {k}")
        assert (buf.pos, buf.full, buf.size()) == (ref.pos, ref.full, ref.upper()) == ((k + 1) % cap, k + 1 >= cap, min(k + 1, cap))
        if k == 2:
            mask = (np.arange(n) % 3 == 0).astype(np.uint8)
            rows, t1 = step[1] + np.float32(1), rng.uniform(0, 1, n).astype(np.float32)
            time = dict(time=t1) if K == 64 else {}
            buf.observe(_dev(rows), mask=_dev(mask), **{k_: _dev(v) for k_, v in time.items()})
            ref.observe(rows, mask=mask, **time)
            _assert_export(buf.export(), ref.export(), norm, "masked observe")
    assert ref.stats[5, 0] == T and ref.stats[6, 0] == 0 and ref.stats[:, 0].sum() > 100 and ref.full
    st, tot = buf.episode_stats(clear=False), ref.stats.sum(axis=0)
    assert (st["episodes"], st["r"], st["l"], st["ep_im_rew"]) == (int(tot[0]), float(tot[1]), int(tot[2]), float(tot[-1])) and st["n_goal_reached"] == tot[3 + 9]
    assert len(st) == 4 + 14 and (st["ep_im_rew"] != 0) == (K != 1)
    assert buf.episode_stats() == st and buf.episode_stats()["episodes"] == 0 and not buf.export()["stats"].any()   # cleared by the second call
    buf.close()


def test_one_env_one_slot():
    buf, ref = _pair(1, 1, 18, 7)
    assert buf.capacity == 1
    for k, step in enumerate(R.scripted_steps(1, 3, 7, seed=2)):
        _add(buf, ref, step, 18)
        _assert_export(buf.export(), ref.export(), True, f"step {k}")
        assert (buf.pos, buf.full, buf.size()) == (0, True, 1)
    buf.close()


@pytest.mark.parametrize("K", [18, 64])
def test_sample_draws_like_the_reference_and_gathers_the_stored_rows(K, oracle_lib):
    """B = 1 and 257, before the ring is full (3 of 5 slots) and after: the recorded (slot, env) pairs are replay_ref's draws, every field is the exported
    array at those pairs (dones = done * (1 - timeout)); supplied pairs are honoured and do not move the call counter; an empty buffer is refused."""
    from human_robot_gym_amd._lib import HrgError
    n, cap, A = 70, 5, 4
    buf, ref = _pair(n, n * cap, K, A, seed=11)
    buf.record_index = True
    with pytest.raises(HrgError, match="replay: the buffer is empty"):
        buf.sample(4)
    steps = list(R.scripted_steps(n, 9, A, seed=4))
    u01 = oracle_lib.hrgo_test_u01
    for filled in (3, 9):
        for step in steps[:3] if filled == 3 else steps[3:]:
            _add(buf, ref, step, K)
        assert ref.upper() == min(filled, cap) and ref.full == (filled > cap)
        x = buf.export()
        dev_ref = R.Replay(n, n * cap, COLS[K], A, observe_time=K == 64)   # the device's own slots under the restatement's gather
        for key in ("observations", "next_observations", "actions", "rewards", "dones", "timeouts"):
            setattr(dev_ref, key, x[key])
        for B in (1, 257):
            want = ref.draw(u01, 11, B)
            got = buf.sample(B)
            idx = buf.last_index.cpu().numpy()
            np.testing.assert_array_equal(idx, want, err_msg=f"filled {filled} B {B}")
            assert idx[:, 0].max() < ref.upper()
            for field, rows in dev_ref.gather(idx).items():
                g = getattr(got, field).cpu().numpy()
                assert g.dtype == np.float32 and g.shape == rows.shape, (field, g.shape, rows.shape)
                np.testing.assert_array_equal(g.view(np.uint32), rows.view(np.uint32), err_msg=f"filled {filled} B {B}: {field}")
            if B == 257:
                d, to = x["dones"][idx[:, 0], idx[:, 1]] != 0, x["timeouts"][idx[:, 0], idx[:, 1]] != 0
                assert (d & to).any() and (d & ~to).any() and np.array_equal(got.dones.cpu().numpy()[:, 0], (d & ~to).astype(np.float32))
        assert got._fields == ("observations", "actions", "next_observations", "dones", "rewards")
        calls = buf.export()["calls"]
        up = ref.upper()
        mine = np.array([[up - 1, n - 1], [0, 0], [0, 0], [up - 1, 0], [1, 64], [1, 63]], np.int64)   # repeats, both ends, across a wave's and a block's seam
        got = buf.sample(len(mine), indices=_dev(mine))
        np.testing.assert_array_equal(buf.last_index.cpu().numpy(), mine)
        for field, rows in dev_ref.gather(mine).items():
            np.testing.assert_array_equal(getattr(got, field).cpu().numpy(), rows, err_msg=field)
        assert buf.export()["calls"] == calls == ref.calls
        for bad in ([[up, 0]], [[0, n]], [[-1, 0]], [[0, -1]]):
            with pytest.raises(IndexError, match="indices"):
                buf.sample(1, indices=_dev(np.array(bad, np.int64)))
        with pytest.raises(ValueError, match="indices"):
            buf.sample(2, indices=_dev(mine))   # B and the pairs disagree
    with pytest.raises(ValueError, match="batch_size"):
        buf.sample(0)
    buf.close()


@pytest.mark.parametrize("squash", [None, 0.5, 3.0])
def test_normalised_view_against_the_float64_restatement(squash):
    """800 rows x (63 columns + time) = 51200 values, std from [0.1, 10]: every value within one float32 ulp of the float64 numpy restatement rounded to
    float32, fewer than 1 in 1000 different at all (a condition; see the module docstring).  Rows of a partial last block, and the current rows."""
    from human_robot_gym_amd.replay import ReplayBuffer, build_replay_desc
    rng = np.random.RandomState(1)
    m, K = 800, 64
    mean, std = rng.uniform(-1, 1, K), rng.uniform(0.1, 10, K)
    buf = ReplayBuffer(build_replay_desc(70, 70, COLS[64], observe_time=True, mean=mean, std=std, squash_factor=squash))
    for m_ in (m, 1, 70):
        rows, time = rng.uniform(-1, 1, (m_, 64)).astype(np.float32), rng.uniform(0, 1, m_).astype(np.float32)
        got = buf.view(_dev(rows), time=_dev(time)).cpu().numpy()
        want = R.view(rows, COLS[64], time, mean, std, squash)
        assert got.shape == (m_, K) and got.dtype == np.float32
        if m_ == m:
            _assert_normalised_close(got, want, f"squash {squash}")
            slip = R.view(rows, COLS[64], time, mean, std, squash, dtype=np.float32)
            assert (R.ulp_distance(slip, want) != 0).mean() > 0.05   # what the cap is there to catch
        else:
            assert R.ulp_distance(got, want).max() <= 1
    buf.observe(_dev(rows), time=_dev(time))
    assert R.ulp_distance(buf.observation().cpu().numpy(), want).max() <= 1
    with pytest.raises(ValueError, match="time column"):
        buf.view(_dev(rows))
    with pytest.raises(ValueError, match="expected a contiguous"):
        buf.view(_dev(rows[:, :63]), time=_dev(time))
    buf.close()


@pytest.mark.parametrize("K", [1, 18])
def test_plain_view_is_the_column_selection(K):
    from human_robot_gym_amd.replay import ReplayBuffer, build_replay_desc
    buf = ReplayBuffer(build_replay_desc(70, 350, COLS[K]))
    for m in (1, 70, 259):   # one wave of one block; a half-full last block; more rows than envs, a last block with three waves
        rows = np.random.RandomState(m).uniform(-1, 1, (m, 64)).astype(np.float32)
        got = buf.view(_dev(rows))
        assert tuple(got.shape) == (m, K)
        np.testing.assert_array_equal(got.cpu().numpy(), rows[:, COLS[K]])
    buf.close()


def _raw_desc(**k):
    d = ReplayDesc()
    d.n_envs, d.capacity, d.act_dim, d.n_obs_cols = 2, 3, 7, 18
    for c in range(18):
        d.obs_cols[c] = c
    for name, v in k.items():
        if name == "col":
            d.obs_cols[v[0]] = v[1]
        elif name == "std0":
            d.normalize = 1
            for c in range(18):
                d.std[c] = 1.0
            d.std[v[0]] = v[1]
        else:
            setattr(d, name, v)
    return d


def test_abi_refusals():
    from human_robot_gym_amd._lib import HrgError, load_library
    from human_robot_gym_amd.replay import ReplayBuffer
    INVALID = CONST["HRG_ERR_INVALID"]
    cases = [(dict(n_envs=0), "n_envs and capacity"), (dict(capacity=0), "n_envs and capacity"), (dict(n_envs=-4), "n_envs and capacity"), (dict(n_obs_cols=0), "n_obs_cols"),
             (dict(n_obs_cols=65), "n_obs_cols"), (dict(n_obs_cols=64, observe_time=1), "n_obs_cols"), (dict(col=(17, 64)), "column outside"),
             (dict(col=(0, -1)), "column outside"), (dict(act_dim=0), "act_dim"), (dict(act_dim=8), "act_dim"), (dict(squash=1), "squash needs normalize"),
             (dict(std0=(4, 0.0)), "std finite and non-zero"), (dict(std0=(4, float("nan"))), "std finite and non-zero"),
             (dict(std0=(4, 1.0), squash=1, squash_factor=float("inf")), "squash_factor")]
    for bad, text in cases:
        with pytest.raises(HrgError, match=f"hrgym error {INVALID}: replay: .*{text}"):
            ReplayBuffer(_raw_desc(**bad))
    ReplayBuffer(_raw_desc(col=(18, 99), std0=(17, 2.0))).close()   # behind n_obs_cols: not a column
    with pytest.raises(HrgError, match=f"hrgym error {CONST['HRG_ERR_NOMEM']}: replay: device allocation of {(1 << 50) * 4 * 18} bytes failed"):
        ReplayBuffer(_raw_desc(n_envs=1 << 20, capacity=1 << 30))   # 2^50 slots: the allocator declines at once; the message names the request
    n = 2
    buf, timed = ReplayBuffer(_raw_desc()), ReplayBuffer(_raw_desc(observe_time=1))
    a, obs, term, rew, dn, info, imit, sir = next(R.scripted_steps(n, 1, 7, seed=1))
    with pytest.raises(HrgError, match="not both"):
        buf.add_step(_dev(a), _dev(obs), _dev(term), _dev(rew), _dev(dn), _dev(info), imit=_dev(imit), sir=_dev(sir))
    with pytest.raises(HrgError, match="observe_time needs the state imitation rows"):
        timed.add_step(_dev(a), _dev(obs), _dev(term), _dev(rew), _dev(dn), _dev(info), imit=_dev(imit))
    with pytest.raises(ValueError, match="time column"):
        timed.observe(_dev(obs))
    assert buf.export()["pos"] == 0 and timed.export()["pos"] == 0 and buf.pos == 0 and timed.pos == 0
    with pytest.raises(ValueError, match="expected a contiguous"):
        buf.add_step(_dev(a)[:1], _dev(obs), _dev(term), _dev(rew), _dev(dn), _dev(info))
    buf.add_step(_dev(a), _dev(obs), _dev(term), _dev(rew), _dev(dn), _dev(info))
    lib, vp = load_library(), ctypes.c_void_p
    outs = [_dev(np.zeros(s, np.float32)) for s in ((2, 18), (2, 7), (2, 18), (2, 1), (2, 1))]
    ptr = lambda ts: [None if t is None else vp(t.data_ptr()) for t in ts]   # noqa: E731
    assert lib.hrg_replay_sample(buf.h, 0, None, *ptr(outs), None, None) == INVALID and b"batch_size" in lib.hrg_last_error()
    for k in range(5):
        assert lib.hrg_replay_sample(buf.h, 2, None, *ptr(outs[:k] + [None] + outs[k + 1:]), None, None) == INVALID and b"null output" in lib.hrg_last_error(), k
    assert lib.hrg_replay_sample(None, 2, None, *ptr(outs), None, None) == INVALID
    assert lib.hrg_replay_sample(buf.h, 2, None, *ptr(outs), None, None) == 0
    words = (ctypes.c_int64 * 4)()
    assert lib.hrg_replay_size(buf.h, words) == 0 and list(words)[:3] == [1, 0, 1]
    assert words[3] == buf.memory_bytes() == 6 * (2 * 18 * 4 + 7 * 4 + 4 + 2) + 2 * (64 * 4 + 4 + 8 + 4 + 8 * 18) + 64 * (4 + 8 + 8)
    assert lib.hrg_replay_size(buf.h, None) == INVALID and lib.hrg_replay_stats(buf.h, None, 0) == INVALID and lib.hrg_replay_view(buf.h, None, None, 2, None, None) == INVALID
    assert buf.add() is None   # the stand-in for an off-policy loop's own add
    buf.close()
    timed.close()


# ---- the device loop against the host loop --------------------------------------------------------------------------------------------------------
class _Policy:
    """A deterministic stand-in: a fixed float32 linear map and tanh, evaluated with torch on the device (products and a sum per output, row by row: a row's
    outputs do not depend on the other rows of its batch).  Actions lie in [-1, 1], the policy's scale."""

    def __init__(self, K, A, seed=0):
        import torch
        self.W = torch.from_numpy(np.random.RandomState(seed).uniform(-1, 1, (K, A)).astype(np.float32)).cuda()
        self.torch = torch

    def __call__(self, obs):
        return self.torch.tanh((obs[:, :, None] * self.W[None]).sum(1))


def _case(name):
    """(constructor keywords, env count, horizon, steps, buffer_size) of the three end-to-end cases."""
    clips = hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300)
    if name == "reach":
        return dict(env_kwargs=dict(horizon=5, seed=11, shield_type="OFF"), clips=clips), 70, 12, 70 * 8
    if name == "icra-pick-place":
        rng = np.random.RandomState(3)
        return dict(env_id="PickPlaceHumanCart", env_kwargs=dict(horizon=7, seed=11), clips=clips, ik_position_delta=dict(action_limit=0.15),
                    collision_prevention=dict(replace_type=0, n_resamples=20), expert=dict(id="PickPlaceHumanCart", signal_to_noise_ratio=0.98),
                    imitation_reward=dict(alpha=0.25, beta=0.7, iota_m=0.1, iota_g=0.5),
                    obs_norm=dict(mean=rng.uniform(-0.5, 0.5, 11), std=rng.uniform(0.1, 10, 11), squash_factor=0.6)), 6, 17, 6 * 10
    from human_robot_gym_amd import dataset as D
    kw = dict(env_kwargs=dict(horizon=6, seed=3, shield_type="SSM"), clips=clips)
    ds = D.collect_expert_dataset("ReachHuman", 8, 8, expert=dict(id="ReachHuman"), **kw)   # recorded here, as tests/test_dataset_gpu.py records its own
    sir = dict(alpha=0.4, iota=0.01, sim_fn="gaussian", observe_time=True, use_et=True, et_dist=2.0)   # early termination 0.02 away from the demonstration: some episodes end by it
    return dict(dataset=ds, rsi_prob=0.5, state_imitation_reward=sir, **kw), 10, 15, 10 * 9


def _host_steps(env, ref, pol, obs, n_steps, tally):
    """OffPolicyAlgorithm.collect_rollouts through env.step, as SB3 runs it: the policy on the uploaded observations, its action unscaled to the bounds into
    the env, the terminal observation as next observation where done, into replay_ref.  `tally`: per-env Monitor-style sums over the infos of done steps."""
    n, keys, be = env.num_envs, env._info_keys, env._backend
    low, high = env.action_space.low.astype(np.float64), env.action_space.high.astype(np.float64)
    for _ in range(n_steps):
        a = pol(_dev(obs)).cpu().numpy()
        obs, rew, done, infos = env.step(low + 0.5 * (a.astype(np.float64) + 1.0) * (high - low))
        nxt, info, ep_im = obs.copy(), np.zeros((n, R.INFO_DIM), np.int32), np.zeros(n, np.float32)
        timeout = np.array([bool(i.get("TimeLimit.truncated", False)) for i in infos])
        for i in np.nonzero(done)[0]:
            nxt[i] = infos[i]["terminal_observation"]
            info[i] = [int(infos[i].get(k, False)) for k in keys]
            ep_im[i] = infos[i].get("ep_im_rew_mean", 0.0)
            tally[i, 0] += 1
            tally[i, 1] += infos[i]["episode"]["r"]
            tally[i, 2] += infos[i]["episode"]["l"]
            tally[i, 3:3 + R.INFO_DIM] += info[i]
            tally[i, 3 + R.INFO_DIM] += ep_im[i]
        # what Monitor sums is the env's own reward: the wrapper's row where an imitation reward is attached
        r_env = be.sir[:, R.SIR_R_ENV] if env._sir is not None else be.imit[:, R.IMIT_R_ENV] if env._imit_alpha is not None else rew
        ref.store(nxt, obs, a, rew, done, timeout, np.array(r_env, copy=True), info, ep_im)
        ref.cur_obs[:] = env._last_full
        ref.cur_time[:] = be.sir[:, R.SIR_TIME_OBS] if env._observe_time else 0
    return obs


@pytest.mark.parametrize("case", ["reach", "icra-pick-place", "dataset-state-imitation"])
def test_collect_steps_is_the_host_loop(case):
    """Two identically seeded envs with a buffer each: collect_steps (twice: the second call continues in mid-episode) on one, the same policy through
    env.step on the other, replay_ref fed from what step returns.  The device loop's buffer equals the restatement (copies bit for bit, normalised
    observations within the tolerance), the host path's fill is the device loop's buffer bit for bit, episode_stats() equals the sums over the host's infos.
    reach: 70 envs, shield off, horizon 5; icra-pick-place: PickPlaceHumanCart behind the IK front-end and collision prevention, with the expert's imitation reward
    and a squashed obs_norm; dataset-state-imitation: a dataset recorded here, the state imitation reward with its time column and early termination, which ends
    the stored episodes there (the other two cases' end at the time limit)."""
    kw, n, steps, size = _case(case)
    dev_env, host_env = hrg.HipVecEnv(n, **kw), hrg.HipVecEnv(n, **kw)
    A, K = dev_env.action_space.shape[0], dev_env.observation_space.shape[0]
    rb, hb = dev_env.attach_replay(size), host_env.attach_replay(size)
    assert dev_env.replay is rb and (rb.n, rb.capacity, rb.act_dim, rb.obs_dim) == (n, size // n, A, K) and rb.observe_time == (case == "dataset-state-imitation")
    assert steps > rb.capacity > dev_env.horizon
    pol = _Policy(K, A)
    ref = R.Replay(n, size, range(K), A)   # fed with the policy's observations as step returns them: the view is the host's
    obs = host_env.reset()
    ref.observe(host_env._last_full, viewed=obs)
    ref.cur_time[:] = host_env._backend.reset_time if host_env._observe_time else 0
    tally = np.zeros((n, R.STATS_DIM))
    normalised = dev_env._norm is not None
    for part in (5, steps - 5):
        assert dev_env.collect_steps(pol, part) is rb
        obs = _host_steps(host_env, ref, pol, obs, part, tally)
        got, want = rb.export(), ref.export()
        _assert_export(got, want, normalised, f"{case} after {part} more steps")
        _assert_export(hb.export(), got, False, f"{case}: the host path's fill against the device loop's")
    d, to = want["dones"] != 0, want["timeouts"] != 0
    assert want["full"] and np.abs(want["actions"]).max() <= 1 and np.abs(want["actions"]).max() > 0.5
    et = case == "dataset-state-imitation"   # there the episodes end by early termination, ahead of the time limit; in the other two by the time limit
    assert (d & ~to).any() if et else (d & to).any()
    print(f"[replay] {case}: {int((d & to).sum())} stored transitions truncated, {int((d & ~to).sum())} terminated")
    if case == "dataset-state-imitation":
        assert len(set(want["observations"][..., -1].ravel())) > 3 and want["observations"][..., -1].max() <= 1
    np.testing.assert_array_equal(got["stats"], tally)
    st, tot = rb.episode_stats(), tally.sum(axis=0)
    assert st["episodes"] == int(tot[0]) >= 2 * n and st["r"] == float(tot[1]) and st["l"] == int(tot[2]) and st["r"] != 0
    assert list(st)[3:-1] == dev_env._info_keys and [st[k] for k in dev_env._info_keys] == [float(x) for x in tot[3:-1]] and (et or st["TimeLimit.truncated"] > 0)
    assert st["ep_im_rew"] == float(tot[-1]) and (st["ep_im_rew"] != 0) == (case != "reach")
    assert hb.episode_stats() == st
    # the sampler works on what the loop stored
    batch = rb.sample(64)
    assert tuple(batch.observations.shape) == (64, K) and tuple(batch.actions.shape) == (64, A) and tuple(batch.dones.shape) == (64, 1)
    # the device loop left the host accounting behind
    with pytest.raises(RuntimeError, match="step_async after collect_steps"):
        dev_env.step_async(np.zeros((n, A)))
    np.testing.assert_array_equal(dev_env.reset(), host_env.reset())
    o1, r1, d1, _ = dev_env.step(np.zeros((n, A)))
    o2, r2, d2, _ = host_env.step(np.zeros((n, A)))
    np.testing.assert_array_equal(o1, o2)
    np.testing.assert_array_equal(r1, r2)
    dev_env.close()
    host_env.close()


def test_attach_replay_refusals_and_reseeding(tmp_path):
    clips = hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300)
    kw = dict(env_kwargs=dict(horizon=3, seed=11, shield_type="OFF"), clips=clips)
    env = hrg.HipVecEnv(2, monitor_dir=str(tmp_path), **kw)
    with pytest.raises(NotImplementedError, match="attach_replay"):
        env.collect_steps(None, 1)
    for bad, text in ((dict(handle_timeout_termination=False), "handle_timeout_termination"), (dict(optimize_memory_usage=True), "optimize_memory_usage")):
        with pytest.raises(NotImplementedError, match=f"attach_replay\\({text}"):
            env.attach_replay(100, **bad)
    assert env.replay is None
    rb = env.attach_replay(101)
    assert (rb.capacity, rb.desc.seed) == (50, 11)
    with pytest.raises(NotImplementedError, match="monitor_dir"):
        env.collect_steps(None, 1)
    env.reset()
    env.step(np.zeros((2, 7)))   # the host path fills it, Monitor csv or not
    assert rb.size() == 1
    env.seed(12)   # a rebuilt batch carries a new, empty buffer of the same shape
    assert env.replay is not rb and (env.replay.capacity, env.replay.size(), env.replay.desc.seed) == (50, 0, 12)
    env.close()
    env = hrg.HipVecEnv(2, goal_env=True, **kw)
    with pytest.raises(NotImplementedError, match="attach_replay: goal_env.*attach_her"):
        env.attach_replay(100)
    env.close()
    mixed = hrg.make_mixed_vec_env(2, tasks=hrg.ICRA_TASKS[:2], n_clips=3)
    with pytest.raises(NotImplementedError, match="attach_replay: the mixed batch"):
        mixed.attach_replay(100)
    mixed.close()


def test_the_config_path_attaches_the_buffer_for_sac_on_flat_observations_only():
    from types import SimpleNamespace as NS

    def config(algorithm, **wrappers):
        return NS(robot=NS(name="Schunk"), wrappers=NS(**wrappers), environment=NS(env_id="ReachHuman", horizon=12, shield_type="OFF", seed=5),
                  run=NS(n_envs=4, seed=5, env_type="env", obs_keys=None, expert_obs_keys=None, start_index=0, monitor_dir=None, monitor_kwargs=None,
                         vec_env_kwargs=dict(clips=hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300))), algorithm=algorithm)
    norm = NS(dataset_name=None, squash_factor=None, allow_different_observation_shapes=False, mean=[0.1] * 18, std=[2.0] * 18)
    env = hrg.create_training_vec_env(config(NS(name="SAC", buffer_size=1000, optimize_memory_usage=False, replay_buffer_kwargs=None), dataset_obs_norm=norm))
    rb = env.replay
    assert rb is not None and env.rollout is None and (rb.n, rb.capacity, rb.act_dim, rb.obs_dim, rb.desc.normalize, rb.desc.squash) == (4, 250, 7, 18, 1, 0)
    assert list(rb.desc.obs_cols[:18]) == list(range(18)) and list(rb.desc.std[:18]) == [2.0] * 18
    env.close()
    env = hrg.create_training_vec_env(config(NS(name="PPO", n_steps=16, gamma=0.98, gae_lambda=0.9, batch_size=64)))
    assert env.replay is None and env.rollout is not None
    env.close()
    for bad in (dict(optimize_memory_usage=True), dict(replay_buffer_kwargs=NS(handle_timeout_termination=False))):
        with pytest.raises(NotImplementedError, match="attach_replay"):
            hrg.create_training_vec_env(config(NS(**dict(dict(name="SAC", buffer_size=1000), **bad))))
