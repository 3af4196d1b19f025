"""The PPO rollout buffer, host side: self-checks of tests/rollout_ref.py (the numpy float32 restatement the device is compared with in
tests/test_rollout_gpu.py), the descriptor's refusals, the config translation, the ABI and where its header is compiled.  No GPU."""
from types import SimpleNamespace as NS

import numpy as np
import pytest

import rollout_ref as R

COLS = list(range(18))   # the PPO layout: object-state, goal_difference


def _filled(n, T, gamma, lam, seed, done):
    """A full reference buffer: rewards, values and last values uniform in [0, 1)."""
    rng = np.random.RandomState(seed)
    ro = R.Rollout(n, T, COLS, gamma=gamma, gae_lambda=lam)
    ro.observe(np.zeros((n, 64), np.float32))
    for t, step in enumerate(R.scripted_steps(n, T, 7, seed, done=done)):
        a, v, lp, tv, obs, rew, dn, info = step
        ro.add(a, rng.uniform(0, 1, n).astype(np.float32), lp, None, obs, rng.uniform(0, 1, n).astype(np.float32), dn, info)
    return ro, rng.uniform(0, 1, n).astype(np.float32)


@pytest.mark.parametrize("T,n", [(1, 70), (5, 70), (64, 70)])
def test_gae_with_lambda_one_is_the_discounted_reward_to_go(T, n):
    """gae_lambda = 1, no episode boundary: advantage[t] + value[t] = sum_k gamma^(k-t) r_k + gamma^(T-t) last_value, here summed in float64.  rtol 1e-5:
    float32 rounding over about 4 T operations on positive terms."""
    gamma = 0.99
    ro, last = _filled(n, T, gamma, 1.0, seed=T, done=np.zeros((T, n)))
    ro.flags[:] = 0   # (the observe before the first step made slot 0 an episode start; the recursion never reads that flag)
    ro.compute(last)
    want = np.zeros((T, n))
    acc = last.astype(np.float64)
    for t in reversed(range(T)):
        acc = ro.rewards[t].astype(np.float64) + gamma * acc
        want[t] = acc
    err = np.abs(ro.returns - want) / np.abs(want)
    print(f"[rollout_ref] T = {T}: largest relative error of the float32 returns {err.max():.3g}")
    np.testing.assert_allclose(ro.returns, want, rtol=1e-5)
    np.testing.assert_allclose(ro.advantages, want - ro.values, rtol=0, atol=1e-5 * np.abs(want).max())
    assert ro.returns.dtype == np.float32 and ro.advantages.dtype == np.float32


def test_an_episode_boundary_stops_the_recursion():
    """Slot 3 starts an episode (the step in slot 2 was done): the advantages of slots 0..2 do not depend on anything from slot 3 on, nor on the last
    values; with the boundary removed they do."""
    n, T = 4, 6
    done = np.zeros((T, n))
    done[2] = 1
    a, last = _filled(n, T, 0.99, 0.9, seed=1, done=done)
    b, _ = _filled(n, T, 0.99, 0.9, seed=1, done=done)
    assert np.all(a.episode_starts[3] == 1) and np.all(a.episode_starts[4:] == 0) and np.all(a.episode_starts[0] == 1)
    b.rewards[3:] += 5
    b.values[3:] -= 2
    a.compute(last)
    b.compute(last + 7)
    np.testing.assert_array_equal(a.advantages[:3], b.advantages[:3])
    assert np.all(a.advantages[3:] != b.advantages[3:])
    np.testing.assert_array_equal(a.advantages[2], a.rewards[2] - a.values[2])   # delta alone: nothing flows over the boundary
    c, _ = _filled(n, T, 0.99, 0.9, seed=1, done=np.zeros((T, n)))
    d, _ = _filled(n, T, 0.99, 0.9, seed=1, done=np.zeros((T, n)))
    d.rewards[3:] += 5
    c.compute(last)
    d.compute(last)
    assert np.all(c.advantages[:3] != d.advantages[:3])
    # the flag of the step after the last slot stops the last values
    e, _ = _filled(n, T, 0.99, 0.9, seed=1, done=np.vstack([np.zeros((T - 1, n)), np.ones((1, n))]))
    e.compute(last)
    np.testing.assert_array_equal(e.advantages[T - 1], e.rewards[T - 1] - e.values[T - 1])


def test_only_a_truncated_done_step_carries_the_terminal_value():
    n, T = 6, 1
    ro = R.Rollout(n, T, COLS, gamma=0.9)
    ro.observe(np.zeros((n, 64), np.float32))
    reward = np.linspace(-1, 1, n).astype(np.float32)
    tv = np.linspace(0.3, 0.8, n).astype(np.float32)
    done = np.array([1, 1, 0, 0, 1, 1], np.uint8)
    info = np.zeros((n, R.INFO_DIM), np.int32)
    info[:, R.INFO_TRUNCATED] = [1, 0, 1, 0, 1, 0]   # env 0, 4: truncated; 1, 5: terminated; 2: the column set on a step that is not done
    z = np.zeros(n, np.float32)
    ro.add(np.zeros((n, 7), np.float32), z, z, tv, np.zeros((n, 64), np.float32), reward, done, info)
    want = reward.copy()
    for e in (0, 4):
        want[e] = np.float32(reward[e] + np.float32(np.float32(0.9) * tv[e]))
    np.testing.assert_array_equal(ro.rewards[0], want)
    assert np.all(ro.rewards[0][[0, 4]] != reward[[0, 4]])
    np.testing.assert_array_equal(ro.stats[:, 1], np.where(done != 0, reward.astype(np.float64), 0.0))   # the episode return is Monitor's: no bootstrap term
    np.testing.assert_array_equal(ro.stats[:, 0], done)
    no_tv = R.Rollout(n, T, COLS, gamma=0.9)
    no_tv.add(np.zeros((n, 7), np.float32), z, z, None, np.zeros((n, 64), np.float32), reward, done, info)
    np.testing.assert_array_equal(no_tv.rewards[0], reward)


def test_the_flat_order_and_the_episode_accumulators():
    n, T = 3, 4
    ro = R.Rollout(n, T, COLS)
    first = np.random.RandomState(0).uniform(-1, 1, (n, 64)).astype(np.float32)
    ro.observe(first)
    done = np.array([[0, 1, 0], [0, 1, 0], [1, 0, 0], [0, 0, 0]])
    steps = list(R.scripted_steps(n, T, 7, seed=2, done=done))
    for s in steps:
        ro.add(*s)
    x = ro.export()
    for e in range(n):
        for t in range(T):
            i = e * T + t   # swap_and_flatten
            np.testing.assert_array_equal(x["observations"][i], (first if t == 0 else steps[t - 1][4])[e, COLS])
            np.testing.assert_array_equal(x["actions"][i], steps[t][0][e])
            assert x["values"][i] == steps[t][1][e] and x["episode_starts"][i] == (1 if t == 0 else done[t - 1, e])
    np.testing.assert_array_equal(x["stats"][:, 0], [1, 2, 0])
    np.testing.assert_array_equal(x["stats"][:, 2], [3, 2, 0])
    r = np.array([s[5] for s in steps], np.float64)
    np.testing.assert_array_equal(x["stats"][:, 1], [r[0, 0] + r[1, 0] + r[2, 0], r[0, 1] + r[1, 1], 0])
    np.testing.assert_array_equal(x["stats"][1, 3:], steps[0][7][1].astype(np.float64) + steps[1][7][1])
    np.testing.assert_array_equal(x["run_length"], [1, 2, 4])
    np.testing.assert_array_equal(x["run_return"], [r[3, 0], r[2, 1] + r[3, 1], r[0, 2] + r[1, 2] + r[2, 2] + r[3, 2]])
    ro.reset()   # rollout_buffer.reset(): the position only
    y = ro.export()
    assert y["pos"] == 0 and np.array_equal(y["flags"], x["flags"]) and np.array_equal(y["stats"], x["stats"]) and np.array_equal(y["cur_obs"], steps[-1][4])


def test_bit_equality_tells_a_contracted_recursion_apart():
    """What the device tests rely on: the recursion with fused multiply-adds gives other bits than the float32 restatement (and is close to it)."""
    n, T = 130, 64
    ro, last = _filled(n, T, 0.99, 0.9, seed=3, done=None)
    ro.compute(last)
    fused = R.gae_with_fma(ro, last)
    differ = ro.advantages.view(np.uint32) != fused.view(np.uint32)
    assert differ.mean() > 0.05
    np.testing.assert_allclose(fused, ro.advantages, rtol=0, atol=1e-5)


def test_build_rollout_desc_and_its_refusals():
    from human_robot_gym_amd.rollout import build_rollout_desc
    d = build_rollout_desc(4096, 64, COLS, act_dim=7, gamma=0.99, gae_lambda=0.9)
    assert (d.n_envs, d.n_steps, d.gamma, d.gae_lambda, d.act_dim, d.n_obs_cols) == (4096, 64, 0.99, 0.9, 7, 18)
    assert list(d.obs_cols[:18]) == COLS and not any(d.obs_cols[18:])
    for bad in (dict(n_envs=0), dict(n_steps=0), dict(act_dim=0), dict(act_dim=8), dict(gamma=-0.1), dict(gamma=1.01), dict(gae_lambda=-0.1), dict(gae_lambda=1.5),
                dict(gamma=float("nan")), dict(obs_cols=[64]), dict(obs_cols=[-1, 3])):
        with pytest.raises(ValueError, match="rollout:"):
            build_rollout_desc(**dict(dict(n_envs=2, n_steps=3, obs_cols=COLS), **bad))
    for cols in ([], list(range(64)) + [0]):
        with pytest.raises(NotImplementedError, match="one value per lane"):
            build_rollout_desc(2, 3, cols)
    assert build_rollout_desc(2, 3, range(64), gamma=1, gae_lambda=0).n_obs_cols == 64


def test_rollout_kwargs_from_config():
    import human_robot_gym_amd as hrg
    from human_robot_gym_amd.training_utils import rollout_kwargs_from_config
    ppo = NS(name="PPO", n_steps=64, gamma=0.99, gae_lambda=0.9, batch_size=64)   # training/config/algorithm/ppo.yaml
    assert rollout_kwargs_from_config(NS(run=NS(env_type="env", n_envs=8), algorithm=ppo)) == dict(n_steps=64, gamma=0.99, gae_lambda=0.9)
    assert hrg.rollout_kwargs_from_config is rollout_kwargs_from_config
    assert rollout_kwargs_from_config(NS(run=NS(n_envs=8), algorithm=NS(name="PPO"))) == dict(n_steps=2048, gamma=0.99, gae_lambda=0.95)   # SB3's defaults
    assert rollout_kwargs_from_config(dict(run=dict(env_type="env"), algorithm=dict(name="PPO", n_steps=16))) == dict(n_steps=16, gamma=0.99, gae_lambda=0.95)
    assert rollout_kwargs_from_config(NS(run=NS(env_type="env"), algorithm=NS(name="SAC", gamma=0.99, buffer_size=10))) is None
    assert rollout_kwargs_from_config(NS(run=NS(env_type="goal_env"), algorithm=ppo)) is None
    assert rollout_kwargs_from_config(NS(run=NS(env_type="env"))) is None


def test_attach_rollout_needs_the_hip_backend_and_the_config_path_skips_other_backends():
    import human_robot_gym_amd as hrg
    from helpers import OracleBackend
    clips = hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300)
    kw = dict(shield_type="OFF", horizon=5)
    env = hrg.HipVecEnv(2, env_kwargs=kw, clips=clips, backend=OracleBackend(hrg.build_model_desc(kw, n_clips=2), clips, 2))
    assert env.rollout is None
    with pytest.raises(NotImplementedError, match="attach_rollout: the rollout kernels run in the HIP library"):
        env.attach_rollout(8)
    with pytest.raises(NotImplementedError, match="attach_rollout"):
        env.collect_rollout(None, None)
    env.close()
    cfg = NS(robot=NS(name="Schunk"), wrappers=NS(), environment=NS(env_id="ReachHuman", horizon=5, shield_type="OFF"),
             run=NS(n_envs=2, seed=5, env_type="env", obs_keys=None, expert_obs_keys=None, start_index=0, monitor_dir=None, monitor_kwargs=None,
                    vec_env_kwargs=dict(clips=clips, backend=lambda desc, cl, n, id0: OracleBackend(desc, cl, n))),
             algorithm=NS(name="PPO", n_steps=8, gamma=0.99, gae_lambda=0.9))
    env = hrg.create_training_vec_env(cfg)   # a CPU backend: no buffer, no error, and the env steps as before
    assert env.rollout is None
    env.reset()
    env.step(np.zeros((2, 7)))
    env.close()


def test_abi_names_and_the_header_stays_in_the_base_translation_unit():
    import ctypes
    from human_robot_gym_amd import _lib
    from human_robot_gym_amd._cstruct import CONST, PROTOTYPES, RolloutDesc
    names = ["hrg_rollout_" + k for k in ("create", "destroy", "view", "observe", "add", "compute", "get", "reset", "stats", "export")]
    assert sorted(k for k in PROTOTYPES if k.startswith("hrg_rollout_")) == sorted(names) and set(names) <= set(_lib.EXPORTS)
    vp = ctypes.c_void_p
    assert PROTOTYPES["hrg_rollout_create"] == (ctypes.c_int, [vp, ctypes.c_int32, vp]) and PROTOTYPES["hrg_rollout_destroy"] == (None, [vp])
    assert PROTOTYPES["hrg_rollout_get"] == (ctypes.c_int, [vp, vp, ctypes.c_int32] + [vp] * 7)
    assert PROTOTYPES["hrg_rollout_add"] == (ctypes.c_int, [vp] * 10) and PROTOTYPES["hrg_rollout_stats"] == (ctypes.c_int, [vp, vp, ctypes.c_int32])
    assert [f for f, _ in RolloutDesc._fields_] == ["n_envs", "n_steps", "gamma", "gae_lambda", "act_dim", "n_obs_cols", "obs_cols"]
    assert ctypes.sizeof(RolloutDesc) == 8 + 16 + 8 + 4 * CONST["HRG_OBS_DIM"]
    base = open(_lib.SRC).read()
    at = base.index('#include "hrgym_rollout.h"')
    assert base.rindex("#if HRG_BASE_TU", 0, at) > base.rindex("#endif", 0, at)   # inside the block that only the base translation unit compiles
    assert at > base.index('#include "hrgym_her.h"')
    assert "// ---- PPO rollout buffer" in open(_lib.SRC.replace("hrgym_hip.hip", "hrgym_host_buffers.h")).read()   # its host side
    for src in _lib.SOURCES[1:]:
        assert "hrgym_rollout.h" not in open(src).read(), src
    assert len(_lib.SOURCES) == 12
    assert any(d.endswith("hrgym_rollout.h") for d in _lib.library_dependencies())   # a dependency of the build
    header = open(_lib.SRC.replace("hrgym_hip.hip", "hrgym_rollout.h")).read()
    assert header.count("#pragma clang fp contract(off)") == 2
