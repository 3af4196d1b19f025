"""numpy restatement of the device evaluation's episode ledger (csrc/hrgym_eval.h), written from SB3 1.5.0's evaluate_policy loop ([UPSTREAM]: from knowledge of
that release) over a Monitor-wrapped VecEnv: episode_count_targets = (n_eval_episodes + i) // n_envs, an env's steps are ignored once its count has met its
target, a finished episode is appended in the order the loop meets it (step by step, env by env), and the appended return and length are Monitor's -- the sums
of the env's own reward (the imitation wrappers sit outside Monitor) and of the steps since the env's last done, whether or not that done was counted.  The
batch may be split into groups of consecutive envs with a target vector each (one parameter set per group).  Self-checked in tests/test_eval.py, the device's
reference in tests/test_eval_gpu.py."""
import numpy as np

OBS_DIM, INFO_DIM, INFO_TRUNCATED = 64, 14, 10
IMIT_R_ENV, IMIT_EP_IM = 1, 4
SIR_R_ENV, SIR_EP_IM = 1, 5
RECORD_DIM = 5 + INFO_DIM
REC_RETURN, REC_LENGTH, REC_STEP, REC_TRUNCATED, REC_INFO, REC_EP_IM = 0, 1, 2, 3, 4, 4 + INFO_DIM


def targets(n_envs, n_policies, n_eval_episodes):
    """episode_count_targets of every group of n_envs / n_policies consecutive envs, concatenated: int64 [n_envs]."""
    m = n_envs // n_policies
    assert m * n_policies == n_envs
    return np.array([(n_eval_episodes + i) // m for _ in range(n_policies) for i in range(m)], dtype=np.int64)


class Ledger:
    def __init__(self, n_envs, n_policies, n_eval_episodes):
        self.n, self.n_policies, self.m = n_envs, n_policies, n_envs // n_policies
        self.targets = targets(n_envs, n_policies, n_eval_episodes)
        self.counts = np.zeros(n_envs, np.int64)
        self.monitor_return, self.monitor_length = np.zeros(n_envs, np.float64), np.zeros(n_envs, np.int64)   # Monitor.rewards summed, len(Monitor.rewards)
        self.t = 0            # steps since the reset
        self.episodes = []    # in append order: dicts of env, r, l, step, truncated, info, ep_im

    def remaining(self):
        return int((self.targets - self.counts).sum())

    def step(self, reward, done, info, imit=None, sir=None):
        """One env.step of the loop: reward f32 [n] (the combined reward where an imitation wrapper is on), done [n], info i32 [n, 14]; imit / sir: the
        imitation rows of the step (at most one), which carry the env's own reward and the episode's imitation reward sum."""
        assert imit is None or sir is None
        r_env = sir[:, SIR_R_ENV] if sir is not None else imit[:, IMIT_R_ENV] if imit is not None else reward
        ep_im = sir[:, SIR_EP_IM] if sir is not None else imit[:, IMIT_EP_IM] if imit is not None else np.zeros(self.n, np.float32)
        self.monitor_return += np.asarray(r_env, np.float32).astype(np.float64)
        self.monitor_length += 1
        for i in range(self.n):
            if not done[i]:
                continue
            if self.counts[i] < self.targets[i]:
                self.episodes.append(dict(env=i, r=float(self.monitor_return[i]), l=int(self.monitor_length[i]), step=self.t, truncated=bool(info[i, INFO_TRUNCATED] != 0),
                                          info=np.array(info[i], np.int64), ep_im=float(np.float32(ep_im[i]))))
                self.counts[i] += 1
            self.monitor_return[i] = 0.0   # Monitor.reset() of the auto-reset
            self.monitor_length[i] = 0
        self.t += 1

    # ---- the results, as evaluate_policy returns them and as the device exports them
    def episode_rewards(self, policy=None):
        return [e["r"] for e in self.episodes if policy is None or e["env"] // self.m == policy]

    def episode_lengths(self, policy=None):
        return [e["l"] for e in self.episodes if policy is None or e["env"] // self.m == policy]

    def column(self, key, policy=None):
        """`key`: env, step, truncated, ep_im, or an index into the info row."""
        pick = [e for e in self.episodes if policy is None or e["env"] // self.m == policy]
        return np.array([e["info"][key] if isinstance(key, int) else e[key] for e in pick])

    def mean_std(self, policy=None):
        r = self.episode_rewards(policy)
        return float(np.mean(r)), float(np.std(r))

    def records(self, max_quota):
        """(counts int32 [n], records float64 [n, max_quota, RECORD_DIM]): record c of env e is the env's c-th appended episode; the rest is zero."""
        rec, c = np.zeros((self.n, max_quota, RECORD_DIM), np.float64), np.zeros(self.n, np.int32)
        for e in self.episodes:
            row = rec[e["env"], c[e["env"]]]
            row[REC_RETURN], row[REC_LENGTH], row[REC_STEP], row[REC_TRUNCATED], row[REC_EP_IM] = e["r"], e["l"], e["step"], float(e["truncated"]), e["ep_im"]
            row[REC_INFO:REC_INFO + INFO_DIM] = e["info"]
            c[e["env"]] += 1
        return c, rec


def done_pattern(n, steps, seed, period=3, p_extra=0.25):
    """uint8 [steps, n]: env e is done at every step t with (t + e) % period == period - 1, and at random further steps: every env finishes at least
    steps // period episodes, of unequal lengths."""
    rng = np.random.RandomState(seed)
    t, e = np.meshgrid(np.arange(steps), np.arange(n), indexing="ij")
    return (((t + e) % period == period - 1) | (rng.uniform(size=(steps, n)) < p_extra)).astype(np.uint8)
