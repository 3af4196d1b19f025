"""numpy restatement of the device replay buffer (csrc/hrgym_replay.h), written from SB3's ReplayBuffer (add, sample, _get_samples with
optimize_memory_usage = False), OffPolicyAlgorithm._store_transition (the terminal observation as next observation of a done step, _last_obs) and
HipVecEnv._view (the columns, the time column, DatasetObsNormWrapper's float64 normalisation rounded to float32 once), plus the episode accumulators Monitor
and the imitation wrappers keep, in float64.  Draws come from the counter hash u01(seed, env, episode, stream, idx) (the oracle's hrgo_test_u01), keyed by
(buffer seed, sample call, index in the batch, STREAM_REPLAY, 0..1).  Self-checked in tests/test_replay.py, the device's reference in tests/test_replay_gpu.py.

Arrays are SB3's, [capacity, n_envs, ...]; `export()` returns them under the keys of ReplayBuffer.export()."""
import numpy as np

STREAM_REPLAY = 11
OBS_DIM, INFO_DIM, INFO_TRUNCATED, ACT_DIM = 64, 14, 10, 7
IMIT_DIM, IMIT_R_ENV, IMIT_EP_IM = 8, 1, 4
SIR_DIM, SIR_R_ENV, SIR_EP_IM, SIR_TIME, SIR_TIME_OBS = 16, 1, 5, 12, 13
STATS_DIM = 4 + INFO_DIM
F32 = np.float32


def scripted_steps(n, steps, act_dim, seed, done=None, p_done=0.3):
    """Synthetic step outputs of n envs: yields (actions f32 [n, act_dim] in [-1, 1], obs, term_obs f32 [n, 64], reward f32 [n], done u8 [n], info i32
    [n, 14], imit f32 [n, 8], sir f32 [n, 16]).  `done`: a [steps, n] pattern instead of the random one.  About half of the done steps are truncations;
    the truncated column is also set on some steps that are not done (stored as it is, and without effect on the sampled dones)."""
    rng = np.random.RandomState(seed)
    for t in range(steps):
        d = (rng.uniform(size=n) < p_done) if done is None else np.asarray(done[t]) != 0
        info = rng.randint(0, 5, (n, INFO_DIM)).astype(np.int32)
        info[:, INFO_TRUNCATED] = np.where(d, rng.uniform(size=n) < 0.5, rng.uniform(size=n) < 0.2)
        yield (rng.uniform(-1, 1, (n, act_dim)).astype(F32), rng.uniform(-1, 1, (n, OBS_DIM)).astype(F32), rng.uniform(-1, 1, (n, OBS_DIM)).astype(F32),
               rng.uniform(-2, 2, n).astype(F32), d.astype(np.uint8), info, rng.uniform(-1, 1, (n, IMIT_DIM)).astype(F32), rng.uniform(0, 1, (n, SIR_DIM)).astype(F32))


def view(rows, cols, time=None, mean=None, std=None, squash_factor=None, dtype=np.float64):
    """HipVecEnv._view of rows of the superset: the columns, the time value behind them, (v - mean) / std and tanh(squash_factor * .) in `dtype` arithmetic
    (float64: the wrapper's; float32: what the device must NOT do), float32 at the end."""
    v = np.asarray(rows, F32)[..., list(cols)]
    if time is not None:
        v = np.concatenate([v, np.asarray(time, F32)[..., None]], axis=-1)
    if mean is not None:
        v = (v.astype(dtype) - np.asarray(mean, dtype)) / np.asarray(std, dtype)
        if squash_factor is not None:
            v = np.tanh(dtype(squash_factor) * v)
        v = v.astype(F32)
    return v


def ulp_distance(a, b):
    """Distance of two float32 arrays in units in the last place (the integer order of IEEE bit patterns)."""
    def key(x):
        i = np.ascontiguousarray(x, F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


class Replay:
    def __init__(self, n, buffer_size, obs_cols, act_dim=ACT_DIM, observe_time=False, mean=None, std=None, squash_factor=None):
        self.n, self.capacity = n, max(int(buffer_size) // n, 1)   # ReplayBuffer.__init__
        self.cols, self.act_dim, self.observe_time = [int(c) for c in obs_cols], act_dim, bool(observe_time)
        self.mean, self.squash_factor = mean, squash_factor
        self.std = None if std is None else np.where(np.asarray(std, np.float64) == 0, 1.0, np.asarray(std, np.float64))
        c, K = self.capacity, len(self.cols) + int(self.observe_time)
        self.observations, self.next_observations = np.zeros((c, n, K), F32), np.zeros((c, n, K), F32)
        self.actions, self.rewards = np.zeros((c, n, act_dim), F32), np.zeros((c, n), F32)
        self.dones, self.timeouts = np.zeros((c, n), np.uint8), np.zeros((c, n), np.uint8)
        self.cur_obs, self.cur_time = np.zeros((n, OBS_DIM), F32), np.zeros(n, F32)   # _last_obs as rows of the superset, and their time values
        self.last_view = self.view(self.cur_obs, self.cur_time)                      # _last_obs as the policy sees it
        self.run_return, self.run_length = np.zeros(n, np.float64), np.zeros(n, np.int32)
        self.stats = np.zeros((n, STATS_DIM), np.float64)
        self.pos, self.full, self.calls = 0, False, 0

    def view(self, rows, time=None):
        return view(rows, self.cols, time if self.observe_time else None, self.mean, self.std, self.squash_factor)

    def upper(self):
        return self.capacity if self.full else self.pos

    def observe(self, obs, time=None, mask=None, viewed=None):
        """After a reset.  `viewed`: the observation the reset returned, instead of the view computed here."""
        m = np.ones(self.n, bool) if mask is None else np.asarray(mask) != 0
        self.cur_obs[m] = obs[m]
        self.cur_time[m] = np.asarray(time, F32)[m] if self.observe_time else 0
        self.last_view[m] = (self.view(obs, time) if viewed is None else viewed)[m]
        self.run_return[m] = 0
        self.run_length[m] = 0

    def store(self, next_view, new_view, actions, reward, done, timeout, r_env, info, ep_im):
        """ReplayBuffer.add on the policy's observations: `next_view` is next_obs with the terminal observation where done (_store_transition), `new_view`
        what the step returned (the new _last_obs).  r_env: what Monitor sums; ep_im: the imitation wrapper's episode sum, read on done steps."""
        p, dn = self.pos, np.asarray(done) != 0
        self.observations[p], self.next_observations[p] = self.last_view, next_view
        self.actions[p], self.rewards[p] = actions, reward
        self.dones[p], self.timeouts[p] = dn, np.asarray(timeout) != 0
        self.last_view = np.array(new_view, F32)
        self.run_return += np.asarray(r_env, F32).astype(np.float64)
        self.run_length += 1
        self.stats[dn, 0] += 1
        self.stats[dn, 1] += self.run_return[dn]
        self.stats[dn, 2] += self.run_length[dn]
        self.stats[dn, 3:3 + INFO_DIM] += np.asarray(info)[dn].astype(np.float64)
        self.stats[dn, 3 + INFO_DIM] += np.asarray(ep_im, F32).astype(np.float64)[dn]
        self.run_return[dn] = 0
        self.run_length[dn] = 0
        self.pos += 1
        if self.pos == self.capacity:
            self.full, self.pos = True, 0

    def add(self, actions, obs, term_obs, reward, done, info, imit=None, sir=None):
        """hrg_replay_add from a step's rows of the superset."""
        assert imit is None or sir is None
        assert sir is not None or not self.observe_time
        dn = np.asarray(done) != 0
        t_next = t_obs = None
        if self.observe_time:
            t_next, t_obs = np.where(dn, sir[:, SIR_TIME], sir[:, SIR_TIME_OBS]), sir[:, SIR_TIME_OBS]
        r_env = sir[:, SIR_R_ENV] if sir is not None else imit[:, IMIT_R_ENV] if imit is not None else reward
        ep_im = sir[:, SIR_EP_IM] if sir is not None else imit[:, IMIT_EP_IM] if imit is not None else np.zeros(self.n, F32)
        nxt = np.where(dn[:, None], term_obs, obs)
        self.store(self.view(nxt, t_next), self.view(obs, t_obs), actions, reward, done, info[:, INFO_TRUNCATED], r_env, info, ep_im)
        self.cur_obs[:] = obs
        self.cur_time[:] = t_obs if self.observe_time else 0

    def draw(self, u01, seed, batch):
        """The (slot, env) pairs of sample call number `self.calls`: int64 [batch, 2]; the call counter moves on."""
        up = self.upper()
        assert up > 0
        idx = np.zeros((batch, 2), np.int64)
        for k in range(batch):
            u0, u1 = u01(seed, self.calls, k, STREAM_REPLAY, 0), u01(seed, self.calls, k, STREAM_REPLAY, 1)
            idx[k] = min(int(np.floor(u0 * up)), up - 1), min(int(np.floor(u1 * self.n)), self.n - 1)
        self.calls += 1
        return idx

    def gather(self, idx):
        """_get_samples at (slot, env) pairs: dict of observations, actions, next_observations, dones [B, 1] = done * (1 - timeout), rewards [B, 1]."""
        s, e = idx[:, 0], idx[:, 1]
        dones = (self.dones[s, e].astype(F32) * (1 - self.timeouts[s, e].astype(F32))).reshape(-1, 1)
        return dict(observations=self.observations[s, e], actions=self.actions[s, e], next_observations=self.next_observations[s, e], dones=dones,
                    rewards=self.rewards[s, e].reshape(-1, 1))

    def export(self):
        out = {k: getattr(self, k).copy() for k in ("observations", "next_observations", "actions", "rewards", "dones", "timeouts", "cur_obs", "cur_time", "run_return",
                                                   "run_length", "stats")}
        out.update(pos=self.pos, full=self.full, calls=self.calls)
        return out
