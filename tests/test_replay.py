"""The uniform replay buffer, host side: self-checks of tests/replay_ref.py (the numpy restatement the device is compared with in
tests/test_replay_gpu.py), the descriptor's refusals, the config translation, the ABI and where its header is compiled.  No GPU."""
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest

import replay_ref as R

COLS = list(range(18))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference", "training", "config_icra_2024", "environment_evaluation", "training")


def _fill(ref, steps, seed, done=None, with_sir=False):
    out = []
    for step in R.scripted_steps(ref.n, steps, ref.act_dim, seed, done=done):
        a, obs, term, rew, dn, info, imit, sir = step
        ref.add(a, obs, term, rew, dn, info, sir=sir if with_sir else None)
        out.append(step)
    return out


def test_the_ring_overwrites_the_oldest_slot_and_upper_follows():
    n, cap = 3, 4
    ref = R.Replay(n, n * cap + 2, COLS)   # buffer_size // n_envs
    assert ref.capacity == cap and ref.upper() == 0 and R.Replay(5, 3, COLS).capacity == 1
    first = np.random.RandomState(0).uniform(-1, 1, (n, 64)).astype(np.float32)
    ref.observe(first)
    steps = []
    for k in range(10):
        steps += _fill(ref, 1, seed=k)
        assert (ref.pos, ref.full, ref.upper()) == ((k + 1) % cap, k + 1 >= cap, min(k + 1, cap))
    for slot in range(cap):   # slot s holds the newest step t with t % cap == s: 8, 9, 6, 7
        t = max(t for t in range(10) if t % cap == slot)
        np.testing.assert_array_equal(ref.actions[slot], steps[t][0])
        np.testing.assert_array_equal(ref.rewards[slot], steps[t][3])
        np.testing.assert_array_equal(ref.observations[slot], steps[t - 1][1][:, COLS])   # the row the step started from: the previous step's obs
    np.testing.assert_array_equal(ref.cur_obs, steps[-1][1])
    one = R.Replay(1, 1, COLS)   # (n, capacity) = (1, 1): full after one add, every add lands in slot 0
    _fill(one, 3, seed=1)
    assert (one.pos, one.full, one.upper()) == (0, True, 1)


def test_next_observation_is_the_terminal_row_only_on_done_steps_with_its_own_time_column():
    n = 6
    ref = R.Replay(n, n * 2, COLS, observe_time=True)
    t0 = np.linspace(0.1, 0.6, n).astype(np.float32)
    first = np.zeros((n, 64), np.float32)
    ref.observe(first, time=t0)
    np.testing.assert_array_equal(ref.last_view[:, -1], t0)
    done = np.array([[1, 0, 1, 0, 1, 0]])
    (step,) = _fill(ref, 1, seed=3, done=done, with_sir=True)
    a, obs, term, rew, dn, info, imit, sir = step
    assert ref.observations.shape == (2, n, 19)
    np.testing.assert_array_equal(ref.observations[0][:, :18], first[:, COLS])
    np.testing.assert_array_equal(ref.observations[0][:, 18], t0)
    for e in range(n):
        row, tcol = (term, R.SIR_TIME) if done[0, e] else (obs, R.SIR_TIME_OBS)
        np.testing.assert_array_equal(ref.next_observations[0, e, :18], row[e, COLS])
        assert ref.next_observations[0, e, 18] == sir[e, tcol]
        assert ref.last_view[e, 18] == sir[e, R.SIR_TIME_OBS] == ref.cur_time[e]
        np.testing.assert_array_equal(ref.last_view[e, :18], obs[e, COLS])   # after auto-reset, never the terminal row
    assert np.all(sir[:, R.SIR_TIME] != sir[:, R.SIR_TIME_OBS])
    # Monitor's return is the row's r_env, not the combined reward; the imitation sum is read on done steps only
    np.testing.assert_array_equal(ref.stats[:, 1], np.where(done[0] != 0, sir[:, R.SIR_R_ENV].astype(np.float64), 0))
    np.testing.assert_array_equal(ref.stats[:, -1], np.where(done[0] != 0, sir[:, R.SIR_EP_IM].astype(np.float64), 0))
    np.testing.assert_array_equal(ref.run_return, np.where(done[0] != 0, 0, sir[:, R.SIR_R_ENV].astype(np.float64)))


def test_sampled_dones_are_zero_exactly_where_a_done_step_was_truncated(oracle_lib):
    n, cap = 70, 5
    ref = R.Replay(n, n * cap, COLS, act_dim=4)
    ref.observe(np.zeros((n, 64), np.float32))
    _fill(ref, 3, seed=5)
    every = np.array([(s, e) for s in range(3) for e in range(n)], np.int64)
    got = ref.gather(every)
    dn, to = ref.dones[:3].reshape(-1) != 0, ref.timeouts[:3].reshape(-1) != 0
    np.testing.assert_array_equal(got["dones"][:, 0], (dn & ~to).astype(np.float32))
    assert (dn & to).sum() > 5 and (dn & ~to).sum() > 5 and (~dn & to).sum() > 5   # truncated, terminated, and the column set on a step that is not done
    assert got["dones"].shape == (210, 1) and got["rewards"].shape == (210, 1) and got["actions"].shape == (210, 4)
    # every drawn slot is < upper, before and after the ring is full; the draws depend on the call, not on the batch size
    u01 = oracle_lib.hrgo_test_u01
    for upper in (3, 5, 5):
        assert ref.upper() == upper
        idx = ref.draw(u01, 11, 300)
        assert idx[:, 0].min() == 0 and idx[:, 0].max() == upper - 1 and idx[:, 1].min() >= 0 and idx[:, 1].max() < n
        assert set(idx[:, 0]) == set(range(upper)) and len(set(idx[:, 1])) > 60
        _fill(ref, 2, seed=upper)
    a, b = R.Replay(n, n * cap, COLS), R.Replay(n, n * cap, COLS)
    for r in (a, b):
        _fill(r, 5, seed=0)
    ia, ib = a.draw(u01, 11, 257), b.draw(u01, 11, 65)
    np.testing.assert_array_equal(ia[:65], ib)
    assert not np.array_equal(b.draw(u01, 11, 65), ib) and not np.array_equal(R.Replay.draw(a, u01, 12, 65), ib) and (a.calls, b.calls) == (2, 2)


def test_the_view_is_the_wrapper_and_float32_arithmetic_would_show():
    """HipVecEnv._view is the restatement's view, bit for bit; the same formula in float32 arithmetic differs from it in far more than 1 value in 1000 (the cap
    the device comparison sets; by many ulps where v - mean cancels): the device test can tell a float32 slip from the allowed rounding-boundary cases."""
    import human_robot_gym_amd as hrg
    from helpers import OracleBackend
    rng = np.random.RandomState(0)
    cols = list(range(63))
    rows, time = rng.uniform(-1, 1, (800, 64)).astype(np.float32), rng.uniform(0, 1, 800).astype(np.float32)
    mean, std = rng.uniform(-1, 1, 64), rng.uniform(0.1, 10, 64)
    for sf in (None, 0.5):
        want = R.view(rows, cols, time, mean, std, sf)
        slip = R.view(rows, cols, time, mean, std, sf, dtype=np.float32)
        assert want.dtype == np.float32 and want.shape == (800, 64)
        d = R.ulp_distance(want, slip)
        print(f"[replay_ref] squash {sf}: float32 arithmetic differs in {np.mean(d != 0):.3f} of {d.size} values, at most {d.max()} ulp")
        assert np.mean(d != 0) > 0.05 > 1e-3
        assert np.all(R.ulp_distance(want, want) == 0)
    assert R.ulp_distance(np.float32([1.0, -0.0, 1e-45]), np.float32([np.nextafter(np.float32(1), np.float32(2)), 0.0, -1e-45])).tolist() == [1, 0, 2]
    clips = hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300)
    kw = dict(shield_type="OFF", horizon=5)
    m18, s18 = rng.uniform(-1, 1, 18), rng.uniform(0.1, 10, 18)
    s18[3] = 0
    env = hrg.HipVecEnv(2, env_kwargs=kw, clips=clips, backend=OracleBackend(hrg.build_model_desc(kw, n_clips=2), clips, 2), obs_norm=dict(mean=m18, std=s18, squash_factor=0.7))
    ref = R.Replay(2, 8, env._cols, mean=m18, std=s18, squash_factor=0.7)
    np.testing.assert_array_equal(env._view(rows[:5]), ref.view(rows[:5]))
    assert ref.std[3] == 1
    env.close()


def test_build_replay_desc_and_its_refusals():
    from human_robot_gym_amd.replay import build_replay_desc, capacity_of
    d = build_replay_desc(4096, 1_000_000, COLS, act_dim=4, seed=7)
    assert (d.n_envs, d.capacity, d.act_dim, d.n_obs_cols, d.observe_time, d.normalize, d.squash, d.seed) == (4096, 244, 4, 18, 0, 0, 0, 7)
    assert list(d.obs_cols[:18]) == COLS and not any(d.obs_cols[18:]) and capacity_of(3, 5) == 1 and build_replay_desc(5, 3, COLS).capacity == 1
    mean, std = np.arange(19.0), np.r_[np.full(18, 2.0), 0.0]
    d = build_replay_desc(2, 10, COLS, observe_time=True, mean=mean, std=std, squash_factor=0.5)
    assert (d.observe_time, d.normalize, d.squash, d.squash_factor) == (1, 1, 1, 0.5) and list(d.mean[:19]) == list(mean)
    assert list(d.std[:19]) == [2.0] * 18 + [1.0] and std[18] == 0   # std == 0 -> 1, on a copy
    assert build_replay_desc(2, 10, range(63), observe_time=True).n_obs_cols == 63 and build_replay_desc(2, 10, range(64)).n_obs_cols == 64
    for kw in (dict(obs_cols=[]), dict(obs_cols=range(64), observe_time=True), dict(obs_cols=list(range(64)) + [0])):   # K < 1, K > 64 with the time column, K > 64
        with pytest.raises(NotImplementedError, match="one value per lane"):
            build_replay_desc(**dict(dict(n_envs=2, buffer_size=10), **kw))
    for kw in (dict(mean=np.zeros(18), std=np.ones(18), observe_time=True), dict(mean=np.zeros(19), std=np.ones(18)), dict(mean=np.zeros(17), std=np.ones(17))):
        with pytest.raises(ValueError, match="replay: statistics of length"):
            build_replay_desc(**dict(dict(n_envs=2, buffer_size=10, obs_cols=COLS), **kw))
    for kw in (dict(n_envs=0), dict(buffer_size=0), dict(act_dim=0), dict(act_dim=8), dict(obs_cols=[64]), dict(obs_cols=[-1, 3]), dict(mean=np.zeros(18)),
               dict(squash_factor=0.5), dict(mean=np.full(18, np.nan), std=np.ones(18))):
        with pytest.raises(ValueError, match="replay:"):
            build_replay_desc(**dict(dict(n_envs=2, buffer_size=10, obs_cols=COLS), **kw))


def test_replay_kwargs_from_config():
    import yaml
    import human_robot_gym_amd as hrg
    from human_robot_gym_amd.training_utils import replay_kwargs_from_config
    assert hrg.replay_kwargs_from_config is replay_kwargs_from_config
    icra = yaml.safe_load(open(os.path.join(GOLDEN, "PP-SAC.yaml")))
    assert icra["algorithm"]["name"] == "SAC" and icra["run"]["env_type"] == "env" and icra["algorithm"]["replay_buffer_kwargs"] is None
    assert replay_kwargs_from_config(icra) == dict(buffer_size=1_000_000, optimize_memory_usage=False)
    sac = NS(name="SAC", buffer_size=5000, optimize_memory_usage=True, replay_buffer_kwargs=NS(handle_timeout_termination=False))
    assert replay_kwargs_from_config(NS(run=NS(env_type="env"), algorithm=sac)) == dict(buffer_size=5000, optimize_memory_usage=True, handle_timeout_termination=False)
    assert replay_kwargs_from_config(NS(run=NS(n_envs=8), algorithm=NS(name="sac"))) == dict(buffer_size=1_000_000)   # SB3's default
    assert replay_kwargs_from_config(NS(run=NS(env_type="env"), algorithm=NS(name="PPO", n_steps=64, gamma=0.99, gae_lambda=0.9))) is None
    assert replay_kwargs_from_config(NS(run=NS(env_type="goal_env"), algorithm=NS(name="SAC", buffer_size=100, replay_buffer_kwargs=NS(n_sampled_goal=4)))) is None
    assert replay_kwargs_from_config(NS(run=NS(env_type="env"))) is None


def test_attach_replay_needs_the_hip_backend_and_the_config_path_skips_other_backends():
    import human_robot_gym_amd as hrg
    from helpers import OracleBackend
    clips = hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300)
    kw = dict(shield_type="OFF", horizon=5)
    env = hrg.HipVecEnv(2, env_kwargs=kw, clips=clips, backend=OracleBackend(hrg.build_model_desc(kw, n_clips=2), clips, 2))
    assert env.replay is None
    with pytest.raises(NotImplementedError, match="attach_replay: the replay kernels run in the HIP library"):
        env.attach_replay(100)
    with pytest.raises(NotImplementedError, match="attach_replay"):
        env.collect_steps(None, 3)
    env.close()
    cfg = NS(robot=NS(name="Schunk"), wrappers=NS(), environment=NS(env_id="ReachHuman", horizon=5, shield_type="OFF"),
             run=NS(n_envs=2, seed=5, env_type="env", obs_keys=None, expert_obs_keys=None, start_index=0, monitor_dir=None, monitor_kwargs=None,
                    vec_env_kwargs=dict(clips=clips, backend=lambda desc, cl, n, id0: OracleBackend(desc, cl, n))),
             algorithm=NS(name="SAC", buffer_size=1000, optimize_memory_usage=False, replay_buffer_kwargs=None))
    env = hrg.create_training_vec_env(cfg)   # a CPU backend: no buffer, no error, and the env steps as before
    assert env.replay is None
    env.reset()
    env.step(np.zeros((2, 7)))
    env.close()


def test_abi_names_and_the_header_stays_in_the_base_translation_unit():
    import ctypes
    from human_robot_gym_amd import _lib
    from human_robot_gym_amd._cstruct import CONST, PROTOTYPES, ReplayDesc
    names = ["hrg_replay_" + k for k in ("create", "destroy", "view", "observe", "add", "sample", "stats", "export", "size")]
    assert sorted(k for k in PROTOTYPES if k.startswith("hrg_replay_")) == sorted(names) and set(names) <= set(_lib.EXPORTS)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    assert PROTOTYPES["hrg_replay_create"] == (ctypes.c_int, [vp, i32, vp]) and PROTOTYPES["hrg_replay_destroy"] == (None, [vp])
    assert PROTOTYPES["hrg_replay_view"] == (ctypes.c_int, [vp, vp, vp, i32, vp, vp]) and PROTOTYPES["hrg_replay_observe"] == (ctypes.c_int, [vp] * 5)
    assert PROTOTYPES["hrg_replay_add"] == (ctypes.c_int, [vp] * 10) and PROTOTYPES["hrg_replay_sample"] == (ctypes.c_int, [vp, i32] + [vp] * 8)
    assert PROTOTYPES["hrg_replay_stats"] == (ctypes.c_int, [vp, vp, i32]) and PROTOTYPES["hrg_replay_export"] == (ctypes.c_int, [vp] * 13)
    assert PROTOTYPES["hrg_replay_size"] == (ctypes.c_int, [vp, vp])
    assert [f for f, _ in ReplayDesc._fields_] == ["n_envs", "capacity", "act_dim", "n_obs_cols", "obs_cols", "observe_time", "normalize", "squash", "squash_factor", "mean",
                                                   "std", "seed"]
    od = CONST["HRG_OBS_DIM"]
    assert ctypes.sizeof(ReplayDesc) == 16 + 4 * od + 12 + 4 + 8 + 16 * od + 8   # (4 bytes of padding ahead of squash_factor)
    assert CONST["HRG_REPLAY_STATS_DIM"] == 4 + CONST["HRG_INFO_DIM"] == R.STATS_DIM and CONST["HRG_REPLAY_INDEX_DIM"] == 2
    assert (CONST["HRG_SIR_TIME"], CONST["HRG_SIR_TIME_OBS"], CONST["HRG_SIR_R_ENV"], CONST["HRG_SIR_EP_IM"]) == (R.SIR_TIME, R.SIR_TIME_OBS, R.SIR_R_ENV, R.SIR_EP_IM)
    assert (CONST["HRG_IMIT_R_ENV"], CONST["HRG_IMIT_EP_IM"], CONST["HRG_IMIT_DIM"], CONST["HRG_SIR_DIM"]) == (R.IMIT_R_ENV, R.IMIT_EP_IM, R.IMIT_DIM, R.SIR_DIM)
    base = open(_lib.SRC).read()
    at = base.index('#include "hrgym_replay.h"')
    assert base.rindex("#if HRG_BASE_TU", 0, at) > base.rindex("#endif", 0, at)   # inside the block that only the base translation unit compiles
    assert at > base.index('#include "hrgym_rollout.h"')
    assert "// ---- uniform replay buffer" in open(_lib.SRC.replace("hrgym_hip.hip", "hrgym_host_buffers.h")).read()   # its host side
    for src in _lib.SOURCES[1:]:
        assert "hrgym_replay.h" not in open(src).read(), src
    assert len(_lib.SOURCES) == 12
    assert any(os.path.basename(d) == "hrgym_replay.h" for d in _lib.library_dependencies())   # a dependency of the build
    header = open(_lib.SRC.replace("hrgym_hip.hip", "hrgym_replay.h")).read()
    assert "STREAM_REPLAY = 11" in header and R.STREAM_REPLAY == 11
    assert "__shared__" not in header and "atomic" not in header.replace("no atomics", "")
