"""numpy float32 restatement of the device rollout buffer (csrc/hrgym_rollout.h), written from SB3's RolloutBuffer (add, compute_returns_and_advantage,
swap_and_flatten) and OnPolicyAlgorithm.collect_rollouts (the bootstrap of time-limit truncations, _last_obs, _last_episode_starts), plus the episode
accumulators Monitor and the logging callback keep, in float64.  Self-checked in tests/test_rollout.py, the device's reference in tests/test_rollout_gpu.py.

Arrays are SB3's, [n_steps, n_envs, ...]; `export()` returns them in the flat order i = env * n_steps + step under the keys of RolloutBuffer.export()."""
import numpy as np

OBS_DIM, INFO_DIM, INFO_TRUNCATED, ACT_DIM = 64, 14, 10, 7
STATS_DIM = 3 + INFO_DIM
F32 = np.float32


def scripted_steps(n, T, act_dim, seed, done=None, p_done=0.3):
    """Synthetic policy outputs and step outputs of n envs over T steps: yields (actions f32 [n, act_dim], values, log_probs, terminal_values f32 [n],
    obs f32 [n, 64], reward f32 [n], done u8 [n], info i32 [n, 14]).  `done`: a [T, n] pattern instead of the random one.  About half of the done steps
    are truncations; the truncated column is also set on some steps that are not done (which must not bootstrap)."""
    rng = np.random.RandomState(seed)
    for t in range(T):
        d = (rng.uniform(size=n) < p_done) if done is None else np.asarray(done[t]) != 0
        info = rng.randint(0, 5, (n, INFO_DIM)).astype(np.int32)
        info[:, INFO_TRUNCATED] = np.where(d, rng.uniform(size=n) < 0.5, rng.uniform(size=n) < 0.2)
        yield (rng.uniform(-1.5, 1.5, (n, act_dim)).astype(F32), rng.uniform(-1, 1, n).astype(F32), rng.uniform(-3, 0, n).astype(F32), rng.uniform(-1, 1, n).astype(F32),
               rng.uniform(-1, 1, (n, OBS_DIM)).astype(F32), rng.uniform(-2, 2, n).astype(F32), d.astype(np.uint8), info)


class Rollout:
    def __init__(self, n, T, obs_cols, act_dim=ACT_DIM, gamma=0.99, gae_lambda=0.95):
        self.n, self.T, self.cols, self.act_dim = n, T, [int(c) for c in obs_cols], act_dim
        self.gamma, self.gae_lambda = float(gamma), float(gae_lambda)
        K = len(self.cols)
        self.observations, self.actions = np.zeros((T, n, K), F32), np.zeros((T, n, act_dim), F32)
        self.rewards, self.values, self.log_probs, self.episode_starts, self.advantages, self.returns = (np.zeros((T, n), F32) for _ in range(6))
        self.cur_obs, self.flags = np.zeros((n, OBS_DIM), F32), np.zeros(n, F32)   # _last_obs (as rows of the superset), _last_episode_starts
        self.run_return, self.run_length = np.zeros(n, np.float64), np.zeros(n, np.int32)
        self.stats = np.zeros((n, STATS_DIM), np.float64)
        self.pos, self.computed = 0, False

    def view(self, rows):
        return np.asarray(rows)[..., self.cols]

    def observe(self, obs, mask=None):
        m = np.ones(self.n, bool) if mask is None else np.asarray(mask) != 0
        self.cur_obs[m] = obs[m]
        self.flags[m] = 1
        self.run_return[m] = 0
        self.run_length[m] = 0

    def add(self, actions, values, log_probs, terminal_values, obs, reward, done, info):
        assert self.pos < self.T
        t, dn = self.pos, np.asarray(done) != 0
        rewards = np.array(reward, F32)
        if terminal_values is not None:   # collect_rollouts: rewards[idx] += self.gamma * terminal_value, where done and TimeLimit.truncated
            boot = dn & (info[:, INFO_TRUNCATED] != 0)
            rewards[boot] = rewards[boot] + F32(self.gamma) * np.asarray(terminal_values, F32)[boot]
        self.observations[t] = self.view(self.cur_obs)
        self.actions[t], self.values[t], self.log_probs[t] = actions, values, log_probs
        self.episode_starts[t], self.rewards[t] = self.flags, rewards
        self.cur_obs[:] = obs   # the row after auto-reset
        self.flags[:] = dn
        self.run_return += np.asarray(reward, F32).astype(np.float64)   # Monitor: without the bootstrap term
        self.run_length += 1
        self.stats[dn, 0] += 1
        self.stats[dn, 1] += self.run_return[dn]
        self.stats[dn, 2] += self.run_length[dn]
        self.stats[dn, 3:] += info[dn].astype(np.float64)
        self.run_return[dn] = 0
        self.run_length[dn] = 0
        self.pos += 1
        self.computed = False

    def compute(self, last_values):
        """compute_returns_and_advantage(last_values, dones = the flags), every operation a float32 one in SB3's order."""
        assert self.pos == self.T
        g, gl = F32(self.gamma), F32(self.gamma * self.gae_lambda)   # (the product in double, as Python takes it)
        one, last = F32(1), np.zeros(self.n, F32)
        for t in reversed(range(self.T)):
            if t == self.T - 1:
                nnt, nv = one - self.flags, np.asarray(last_values, F32)
            else:
                nnt, nv = one - self.episode_starts[t + 1], self.values[t + 1]
            delta = (self.rewards[t] + (g * nv) * nnt) - self.values[t]
            last = delta + (gl * nnt) * last
            assert delta.dtype == F32 and last.dtype == F32
            self.advantages[t] = last
        self.returns[:] = self.advantages + self.values
        self.computed = True

    def reset(self):
        self.pos, self.computed = 0, False

    @staticmethod
    def flat(a):
        """swap_and_flatten: [T, n, ...] -> [n * T, ...], i = env * T + step."""
        return np.ascontiguousarray(np.swapaxes(a, 0, 1)).reshape((a.shape[0] * a.shape[1],) + a.shape[2:])

    def export(self):
        out = {k: self.flat(getattr(self, k)) for k in ("observations", "actions", "rewards", "values", "log_probs", "episode_starts", "advantages", "returns")}
        out.update(cur_obs=self.cur_obs.copy(), flags=self.flags.copy(), run_return=self.run_return.copy(), run_length=self.run_length.copy(), stats=self.stats.copy(),
                   pos=self.pos, computed=self.computed)
        return out


def gae_with_fma(ro, last_values):
    """The recursion of `Rollout.compute` as a compiler that contracts a * b + c would run it: each multiply-add pair rounded once (through float64, where the
    product of two float32 is exact).  Returns the advantages [T, n].  Not a reference: tests use it to show that bit equality tells the two apart."""
    f = lambda a, b, c: (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(F32)   # noqa: E731
    g, gl = F32(ro.gamma), F32(ro.gamma * ro.gae_lambda)
    last, adv = np.zeros(ro.n, F32), np.zeros((ro.T, ro.n), F32)
    for t in reversed(range(ro.T)):
        nnt, nv = (F32(1) - ro.flags, np.asarray(last_values, F32)) if t == ro.T - 1 else (F32(1) - ro.episode_starts[t + 1], ro.values[t + 1])
        delta = f(g * nv, nnt, ro.rewards[t]) - ro.values[t]
        last = f(gl * nnt, last, delta)
        adv[t] = last
    return adv
