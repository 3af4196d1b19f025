"""What the rollout and the replay buffer share on the device (csrc/hrgym_buffer.h): the episode tracker and the policy's view of rows, driven through both
classes with the same synthetic tensors -- no env.  The two buffers must agree bit for bit, and with a restatement in numpy.  -m gpu.

Sizes: 3 envs and 6 steps for the tracker (an env done on its first step, one done on two consecutive steps, one never done and observed again under a mask
after the third step); 1, 4 and 5 rows for the view (blocks of four rows: a short one, a full one, one row spilling into a second block) at observations of 1
and 64 values and, for the replay buffer, 63 values and the time column."""
import numpy as np
import pytest

from human_robot_gym_amd._cstruct import CONST

pytestmark = pytest.mark.gpu

OBS_DIM, INFO_DIM, ACT_DIM = CONST["HRG_OBS_DIM"], CONST["HRG_INFO_DIM"], CONST["HRG_ACT_DIM"]
PERM = [int(c) for c in np.random.RandomState(5).permutation(OBS_DIM)]


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _buffers(n, cols, slots, observe_time=False, rollout=True):
    from human_robot_gym_amd.replay import ReplayBuffer, build_replay_desc
    from human_robot_gym_amd.rollout import RolloutBuffer, build_rollout_desc
    ro = RolloutBuffer(build_rollout_desc(n, slots, cols)) if rollout else None
    return ro, ReplayBuffer(build_replay_desc(n, n * slots, cols, observe_time=observe_time))


def _bits(a):
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def test_tracker_same_in_both_buffers():
    n, T = 3, 6
    rng = np.random.RandomState(11)
    obs = rng.uniform(-1, 1, (T + 1, n, OBS_DIM)).astype(np.float32)
    rew = rng.uniform(-1, 1, (T, n)).astype(np.float32)
    info = rng.randint(0, 5, (T, n, INFO_DIM)).astype(np.int32)
    act = rng.uniform(-1, 1, (T, n, ACT_DIM)).astype(np.float32)
    done = np.zeros((T, n), np.uint8)
    done[0, 0] = 1                # on its very first step
    done[2, 1] = done[3, 1] = 1   # twice in a row
    again = rng.uniform(-1, 1, (n, OBS_DIM)).astype(np.float32)   # what the never-done env is observed with after the third step
    mask = np.array([0, 0, 1], np.uint8)
    ro, rp = _buffers(n, list(range(18)), T)
    ro.observe(_dev(obs[0]))
    rp.observe(_dev(obs[0]))
    val = _dev(np.zeros(n, np.float32))
    for k in range(T):
        o, r, d, i = _dev(obs[k + 1]), _dev(rew[k]), _dev(done[k]), _dev(info[k])
        ro.add_step(_dev(act[k]), val, val, None, o, None, r, d, i)
        rp.add_step(_dev(act[k]), o, o, r, d, i)
        if k == 2:
            ro.observe(_dev(again), mask=_dev(mask))
            rp.observe(_dev(again), mask=_dev(mask))
    a, b = ro.export(), rp.export()
    ro.close()
    rp.close()
    # the restatement: Monitor's sums in float64
    run_ret, run_len, stats = np.zeros(n), np.zeros(n, np.int32), np.zeros((n, 3 + INFO_DIM))
    for k in range(T):
        run_ret, run_len, d = run_ret + rew[k].astype(np.float64), run_len + 1, done[k] != 0
        stats[d] += np.column_stack([np.ones(n), run_ret, run_len, info[k]])[d]
        z = d | (mask != 0) if k == 2 else d   # a done step, and the masked observe after the third, start the sums again
        run_ret[z], run_len[z] = 0.0, 0
    cur = obs[T].copy()
    assert stats[0, 0] == 1 and stats[1, 0] == 2 and stats[2, 0] == 0 and run_len.tolist() == [5, 2, 3]
    for key, want in (("run_return", run_ret), ("run_length", run_len), ("cur_obs", cur)):
        assert a[key].dtype == b[key].dtype == want.dtype, key
        np.testing.assert_array_equal(_bits(a[key]), _bits(b[key]), err_msg=key)
        np.testing.assert_array_equal(_bits(a[key]), _bits(want), err_msg=key)
    assert a["stats"].shape == (n, 3 + INFO_DIM) and b["stats"].shape == (n, 4 + INFO_DIM)
    np.testing.assert_array_equal(_bits(a["stats"]), _bits(np.ascontiguousarray(b["stats"][:, :3 + INFO_DIM])))
    np.testing.assert_array_equal(_bits(a["stats"]), _bits(stats))
    np.testing.assert_array_equal(b["stats"][:, 3 + INFO_DIM], 0.0)   # no imitation rows: nothing in the replay buffer's extra column


@pytest.mark.parametrize("width, observe_time", [(1, False), (64, False), (63, True)])
def test_view_same_in_both_buffers(width, observe_time):
    cols = [37] if width == 1 else PERM[:width]
    ro, rp = _buffers(2, cols, 1, observe_time=observe_time, rollout=not observe_time)
    for m in (1, 4, 5):
        rows = np.arange(m * OBS_DIM, dtype=np.float32).reshape(m, OBS_DIM)
        time = np.arange(m, dtype=np.float32) + 0.5
        want = rows[:, cols]
        if observe_time:
            want = np.concatenate([want, time[:, None]], axis=1)
        got = rp.view(_dev(rows), time=_dev(time) if observe_time else None).cpu().numpy()
        assert got.shape == want.shape
        np.testing.assert_array_equal(_bits(got), _bits(np.ascontiguousarray(want)), err_msg=f"replay view of {m} rows")
        if ro is not None:
            np.testing.assert_array_equal(_bits(ro.view(_dev(rows)).cpu().numpy()), _bits(got), err_msg=f"rollout view of {m} rows")
    rp.close()
    if ro is not None:
        ro.close()
