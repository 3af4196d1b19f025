"""numpy restatement of one DAgger step on the device (csrc/hrgym_dagger.h), written from the rules, not from the kernel: the expert's label
(bc.demonstration_actions: clip to the bounds, SB3's scale_action in float64 for SAC, rounded to float32 once), the per-env mixing draw from the counter hash
u01(seed, env, episode, stream, idx) (the oracle's hrgo_test_u01) keyed by (dagger seed, call, global env id, STREAM_DAGGER, 0), the rows the envs execute
(SB3's unscale_action in float64 as collect_steps evaluates it; SB3's float32 clip as collect_rollout does), the action the replay buffer keeps, the per-env
statistics in float64, and the table's ring behind a pinned prefix.  Self-checked in tests/test_dagger.py, the device's reference in tests/test_dagger_gpu.py."""
import numpy as np

STREAM_DAGGER = 16
ACT_DIM = 7
F32 = np.float32


def label(expert, low, high, kind, dtype=np.float64, reciprocal=False):
    """float32 [n, A]: the first A = len(low) columns of the expert's rows as the table stores them.  `dtype` float32: the arithmetic the device must NOT use;
    `reciprocal`: the division as a multiplication by 1 / (high - low) in `dtype` (a variant the float64 result is compared with)."""
    low, high = np.asarray(low, np.float64).astype(dtype), np.asarray(high, np.float64).astype(dtype)
    c = np.clip(np.asarray(expert, np.float64)[:, :len(low)].astype(dtype), low, high)
    if kind == "ppo":
        return c.astype(F32)
    q = (c - low) * (dtype(1.0) / (high - low)) if reciprocal else (c - low) / (high - low)
    return (dtype(2.0) * q - dtype(1.0)).astype(F32)


def draws(u01, seed, call, n, env_id0=0):
    """float64 [n]: env e's draw of step `call`."""
    return np.array([u01(seed, call, env_id0 + e, STREAM_DAGGER, 0) for e in range(n)], np.float64)


def label_inputs(n, act_dim, limit, seed):
    """Expert rows float64 [n, 7] that leave the bounds: motions uniform in 1.3 x the limit, the last of the `act_dim` columns a gripper command of {-1, 0.3, 1};
    and the float32 bounds of the action space as float64."""
    rng = np.random.RandomState(seed)
    x = np.zeros((n, ACT_DIM))
    x[:, :act_dim] = rng.uniform(-1.3 * limit, 1.3 * limit, (n, act_dim))
    x[:, act_dim - 1] = rng.choice([-1.0, 0.3, 1.0], n)
    high = np.array([limit] * (act_dim - 1) + [1.0], F32).astype(np.float64)
    return x, -high, high


class Dagger:
    """The handle and its table.  `pinned`: (observations f32 [p, K], actions f32 [p, A]) or None."""

    def __init__(self, kind, n, K, A, capacity_steps, low, high, seed, env_id0=0, pinned=None):
        assert kind in ("sac", "ppo")
        self.kind, self.n, self.K, self.A, self.capacity_steps, self.seed, self.env_id0 = kind, n, K, A, int(capacity_steps), seed, env_id0
        self.low, self.high = np.asarray(low, np.float64), np.asarray(high, np.float64)
        self.pinned = 0 if pinned is None else len(pinned[0])
        rows = self.pinned + self.capacity_steps * n
        self.observations, self.actions = np.zeros((rows, K), F32), np.zeros((rows, A), F32)
        if pinned is not None:
            self.observations[:self.pinned], self.actions[:self.pinned] = pinned
        self.calls, self.slot = 0, 0
        self.stats = np.zeros((n, 3), np.float64)

    @property
    def n_rows(self):
        return self.pinned + min(self.calls, self.capacity_steps) * self.n

    def slot_rows(self, slot):
        a = self.pinned + slot * self.n
        return slice(a, a + self.n)

    def step(self, u01, view, learner, expert, beta):
        """-> dict(rows f64 [n, 7] executed, kept f32 [n, A], expert bool [n] who drove, label f32 [n, A], slot: the one written)."""
        n, A, lo, hi = self.n, self.A, self.low, self.high
        view, learner = np.asarray(view, F32), np.asarray(learner, F32)
        lab = label(expert, lo, hi, self.kind)
        drove = draws(u01, self.seed, self.calls, n, self.env_id0) < beta
        if self.kind == "sac":
            own = lo + 0.5 * (learner.astype(np.float64) + 1.0) * (hi - lo)   # unscale_action, float64, in this order
            at_label = learner
        else:
            at_label = np.clip(learner, lo.astype(F32), hi.astype(F32))   # float32, as SB3 clips what the env gets
            own = at_label.astype(np.float64)
        rows = np.zeros((n, ACT_DIM))
        rows[:, :A] = np.where(drove[:, None], np.clip(np.asarray(expert, np.float64)[:, :A], lo, hi), own)
        kept = np.where(drove[:, None], lab, learner).astype(F32)
        sl = self.slot_rows(self.slot)
        self.observations[sl], self.actions[sl] = view, lab
        d = at_label.astype(np.float64) - lab.astype(np.float64)
        sq = np.zeros(n)
        for j in range(A):   # ascending
            sq += d[:, j] * d[:, j]
        self.stats += np.stack([np.ones(n), drove.astype(np.float64), sq], axis=1)
        out = dict(rows=rows, kept=kept, expert=drove, label=lab, slot=self.slot)
        self.calls += 1
        self.slot = (self.slot + 1) % self.capacity_steps
        return out
