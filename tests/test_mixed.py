"""Mixed-task batches (BASELINE.json's last configuration: the ICRA-2024 task suite in one batch, icra_2024_run_experiments.sh:4-9)."""
import numpy as np
import pytest

import human_robot_gym_amd as hrg
from human_robot_gym_amd import mixed
from human_robot_gym_amd.model import ENV_DEFAULTS


def test_even_split_and_task_table():
    assert mixed.split_evenly(4096, 4) == [1024] * 4 and len(mixed.ICRA_TASKS) == 6     # the six tasks of icra_2024_run_experiments.sh:4-9
    assert mixed.split_evenly(10, 4) == [3, 3, 2, 2] and sum(mixed.split_evenly(4097, 6)) == 4097
    for env_id, kw in mixed.ICRA_TASKS:
        assert env_id in ENV_DEFAULTS
        assert kw["horizon"] == {"ReachHuman": 100, "CollaborativeLiftingCart": 5000, "CollaborativeStackingCart": 3000}.get(env_id, 1000)   # icra_2024_run_experiments.sh:4-9
        assert kw["shield_type"] == ("PFL" if "Handover" in env_id else "SSM")
        clips = mixed.task_clips(env_id, 2, min_frames=60, max_frames=80)
        assert clips.n_clips == 2


def test_mixed_batch_fails_loudly_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mixed.make_mixed_batch(8)


class _TwoOracles:
    """Backend protocol over two OracleBackends, rows part by part, with the `env_ids` / `slices` a MixedHipVecEnv reads."""

    def __init__(self, parts, horizon, n_clips):
        from helpers import OracleBackend
        self.env_ids, self.slices, self.backends = [], [], []
        r0 = 0
        for env_id, k in parts:
            clips = mixed.task_clips(env_id, n_clips, min_frames=60, max_frames=80)
            desc = hrg.build_model_desc(dict(mixed.task_env_kwargs(env_id), horizon=horizon, shield_type="SSM", seed=1), n_clips=clips.n_clips, env_id=env_id)
            self.backends.append(OracleBackend(desc, clips, k, env_id0=r0))
            self.env_ids.append(env_id)
            self.slices.append(slice(r0, r0 + k))
            r0 += k

    def reset(self):
        return np.concatenate([b.reset() for b in self.backends])

    def step_async(self, actions):
        for b, sl in zip(self.backends, self.slices):
            b.step_async(np.ascontiguousarray(actions[sl]))

    def step_wait(self):
        return tuple(np.concatenate(x) for x in zip(*[b.step_wait() for b in self.backends]))

    def executed_actions(self):
        return np.concatenate([b.executed_actions() for b in self.backends])

    def close(self):
        for b in self.backends:
            b.close()


def test_mixed_vec_env_surface_on_the_oracle_backends(oracle_lib):
    """MixedHipVecEnv over any backend of the protocol: what test_mixed_vec_env_surface asserts on the GPU, row for row, on two CPU oracle batches; and the
    "task" entry does not materialise the lazy info rows."""
    env = mixed.MixedHipVecEnv(_TwoOracles([("ReachHuman", 2), ("PickPlaceHumanCart", 2)], horizon=4, n_clips=2))
    assert env.num_envs == 4 and env.observation_space.shape == (64,) and env.action_space.shape == (7,)
    assert env.task_slices == {"ReachHuman": slice(0, 2), "PickPlaceHumanCart": slice(2, 4)}
    obs = env.reset()
    assert obs.shape == (4, 64) and obs.dtype == np.float32
    assert np.all(obs[env.task_slices["ReachHuman"], 39:53] == 0)              # cube columns: zero for ReachHuman
    assert np.any(obs[env.task_slices["PickPlaceHumanCart"], 47:50] != 0)      # object_pos
    rng = np.random.RandomState(0)
    n_done = 0
    for _ in range(6):
        obs, rew, dones, infos = env.step(rng.uniform(-1, 1, (4, 7)))
        assert [d["task"] for d in infos] == env.get_attr("task") == ["ReachHuman"] * 2 + ["PickPlaceHumanCart"] * 2
        assert all(d._src is not None for d in infos)                           # reading "task" left the rows lazy
        for d, done in zip(infos, dones):
            assert ("terminal_observation" in d) == bool(done)
            if done:
                assert d["terminal_observation"].shape == (64,) and d["episode"]["l"] <= 4
        n_done += int(dones.sum())
    assert n_done >= 4                                                          # horizon 4: every env timed out once
    env.close()
    env2 = mixed.MixedHipVecEnv(_TwoOracles([("ReachHuman", 2), ("PickPlaceHumanCart", 2)], horizon=4, n_clips=2), obs_keys=["robot0_eef_pos", "dist_eef_to_human_head"])
    assert env2.reset().shape == (4, 4) and env2.obs_keys == ["robot0_eef_pos", "dist_eef_to_human_head"]
    env2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("concurrent,tasks", [(True, "ICRA_TASKS"), (False, "ICRA_TASKS"), (True, "ALL_TASKS")])
def test_mixed_batch_equals_the_per_task_batches(concurrent, tasks):
    """Each task's rows of a mixed batch are bit-identical to that task stepped alone (same global env ids, same actions); ALL_TASKS adds the hammering task."""
    import torch
    from human_robot_gym_amd._lib import HipBatch
    tasks = getattr(mixed, tasks)
    n = 7 * len(tasks)
    M = mixed.make_mixed_batch(n, tasks=tasks, n_clips=3, seed=5, concurrent=concurrent)
    assert M.env_ids == [t[0] for t in tasks] and M.n == n
    singles = []
    for (env_id, kw), sl in zip(tasks, M.slices):
        clips = mixed.task_clips(env_id, 3)
        desc = hrg.build_model_desc(dict(mixed.task_env_kwargs(env_id), **dict(kw, seed=5)), n_clips=clips.n_clips, env_id=env_id)
        singles.append(HipBatch(desc, clips, sl.stop - sl.start, env_id0=sl.start))
    obs = M.reset().cpu().numpy()
    for S, sl in zip(singles, M.slices):
        np.testing.assert_array_equal(obs[sl], S.reset().cpu().numpy())
    rng = np.random.RandomState(0)
    for k in range(12):
        a = torch.from_numpy(rng.uniform(-1, 1, (n, 7))).cuda()
        o, r, d, i = [x.cpu().numpy().copy() for x in M.step(a)]
        t = M.term_obs.cpu().numpy()
        for S, sl in zip(singles, M.slices):
            so, sr, sd, si = S.step(a[sl].contiguous())
            np.testing.assert_array_equal(o[sl], so.cpu().numpy(), err_msg=f"step {k}")
            np.testing.assert_array_equal(r[sl], sr.cpu().numpy())
            np.testing.assert_array_equal(d[sl], sd.cpu().numpy())
            np.testing.assert_array_equal(i[sl], si.cpu().numpy())
            np.testing.assert_array_equal(t[sl], S.term_obs.cpu().numpy())
    for S in singles:
        S.close()
    M.close()


@pytest.mark.gpu
def test_mixed_vec_env_surface():
    env = mixed.make_mixed_vec_env(12, env_kwargs=dict(horizon=5), tasks=[(e, dict(k, horizon=5)) for e, k in mixed.ICRA_TASKS], n_clips=2, seed=1)
    assert env.num_envs == 12 and env.observation_space.shape == (64,) and env.action_space.shape == (7,)
    obs = env.reset()
    assert obs.shape == (12, 64) and obs.dtype == np.float32
    assert np.all(obs[env.task_slices["ReachHuman"], 39:53] == 0)              # cube columns: zero for ReachHuman
    assert np.any(obs[env.task_slices["PickPlaceHumanCart"], 47:50] != 0)      # object_pos
    rng = np.random.RandomState(0)
    n_done = 0
    for _ in range(6):
        obs, rew, dones, infos = env.step(rng.uniform(-1, 1, (12, 7)))
        assert [d["task"] for d in infos] == env.get_attr("task")
        for d, done in zip(infos, dones):
            assert ("terminal_observation" in d) == bool(done)
            if done:
                assert d["terminal_observation"].shape == (64,) and d["episode"]["l"] <= 5
        n_done += int(dones.sum())
    assert n_done >= 12                                                         # horizon 5: every env timed out once (a board may also be dropped earlier)
    env2 = mixed.make_mixed_vec_env(8, obs_keys=["robot0_eef_pos", "dist_eef_to_human_head"], n_clips=2)
    assert env2.reset().shape == (8, 4)
    env.close()
    env2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("suite", ["ICRA_TASKS", "ALL_TASKS"])
def test_six_task_mixed_batch_at_4096_envs(suite):
    """BASELINE configs[4] on one GPU: the six ICRA tasks, 4096 envs split evenly, each task's kernel on its own stream.  Size-independent properties over
    40 steps, and every task's rows bit-identical to the task stepped alone at the same global env ids."""
    import torch
    from human_robot_gym_amd._lib import HipBatch
    n = 4096
    tasks = getattr(mixed, suite)   # ALL_TASKS: the six ICRA tasks + CollaborativeHammeringCart, seven kernels in one batch
    M = mixed.make_mixed_batch(n, tasks=tasks, seed=11)
    assert len(M.env_ids) == len(tasks) and M.n == n and [sl.stop - sl.start for sl in M.slices] == mixed.split_evenly(n, len(tasks))
    if suite == "ICRA_TASKS":
        assert [sl.stop - sl.start for sl in M.slices] == [683, 683, 683, 683, 682, 682]
    singles = []
    for (env_id, kw), sl in zip(tasks, M.slices):
        clips = mixed.task_clips(env_id, 13)
        singles.append(HipBatch(hrg.build_model_desc(dict(mixed.task_env_kwargs(env_id), **dict(kw, seed=11)), n_clips=clips.n_clips, env_id=env_id), clips, sl.stop - sl.start, env_id0=sl.start))
    obs = M.reset()
    for S, sl in zip(singles, M.slices):
        assert torch.equal(obs[sl], S.reset())
    gen = torch.Generator(device="cuda"); gen.manual_seed(3)
    crashes = 0
    for k in range(40):
        a = torch.rand((n, 7), generator=gen, device="cuda", dtype=torch.float64) * 2 - 1
        o, r, d, i = M.step(a)
        torch.cuda.synchronize()
        assert torch.isfinite(o).all() and torch.isfinite(r).all()
        crashes += int(i[:, 11].sum())
        for S, sl in zip(singles, M.slices):
            so, sr, sd, si = S.step(a[sl].contiguous())
            assert torch.equal(o[sl], so) and torch.equal(r[sl], sr) and torch.equal(d[sl], sd) and torch.equal(i[sl], si), f"step {k} {S}"
    st = M.slices[M.env_ids.index("CollaborativeStackingCart")]
    assert int(M.info[st, 13].max()) >= 1                 # max_stack_height: the human has put its first cube down somewhere
    assert crashes < 0.01 * n * 40
    for S in singles:
        S.close()
    M.close()
