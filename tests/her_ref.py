"""numpy restatement of the device replay buffer (csrc/hrgym_her.h): the ring rules of the add / observe kernels, the sampler and the reward / done rule of
relabelled transitions (the arithmetic of HipVecEnv.compute_reward / compute_done).  Draws come from the counter hash u01(seed, env, episode, stream, idx)
(the oracle's hrgo_test_u01), keyed by (buffer seed, sample call, index in the batch, STREAM_HER, 0..2).  Self-checked in tests/test_her.py, the device's
reference in tests/test_her_gpu.py."""
import numpy as np

STREAM_HER = 10
OBS_DIM, INFO_DIM, INFO_COLLISION_TYPE, INFO_TRUNCATED = 64, 14, 1, 10
ILLEGAL = 8 | 4 | 16   # HRG_COL_STATIC | HRG_COL_ROBOT | HRG_COL_HUMAN_CRIT
# columns of the observation superset behind the goals (vec_env.HipVecEnv._init_columns) and what a reached state offers as a new goal
AG_COLS = {"reach": list(range(18, 24)), "cube": [30, 31, 32, 47, 48, 49, 39]}
DG_COLS = {"reach": list(range(33, 39)), "cube": [50, 51, 52]}
NEW_GOAL_COLS = {"reach": list(range(18, 24)), "cube": [47, 48, 49]}
PARAMS = dict(goal_dist=0.1, task_reward=1.0, object_gripped_reward=-1.0, reward_shaping=0, collision_reward=0.0, reward_scale=1.0, done_at_success=0, done_at_collision=0)


def goal_distance(kind, ag, dg):
    """The distance success is decided on: row by row, ||ag - dg|| (reach) / ||dg - object_pos|| (cube)."""
    ag, dg = np.atleast_2d(np.asarray(ag, np.float64)), np.atleast_2d(np.asarray(dg, np.float64))
    return np.linalg.norm(ag - dg, axis=-1) if kind == "reach" else np.linalg.norm(dg - ag[:, 3:6], axis=-1)


def reward_done(kind, p, ag, dg, ctype):
    """HumanEnv._compute_reward / _check_done (human_env.py:629-664, 835-858) in FP64: (reward, done)."""
    ag, dg, ctype = np.atleast_2d(np.asarray(ag, np.float64)), np.atleast_2d(np.asarray(dg, np.float64)), np.asarray(ctype)
    dist = goal_distance(kind, ag, dg)
    if kind == "reach":
        r = np.where(dist <= p["goal_dist"], p["task_reward"], -1.0)
        dense = -0.1 * dist
    else:
        e2o = np.linalg.norm(ag[:, 3:6] - ag[:, 0:3], axis=-1)
        r = np.where(dist <= p["goal_dist"], p["task_reward"], np.where(ag[:, 6] != 0, p["object_gripped_reward"], -1.0))
        dense = -(e2o * 0.2 + dist) * 0.1
    if p["reward_shaping"]:
        r = r + 1.0 + dense
    illegal = (ctype & ILLEGAL) != 0
    r = (r + np.where(illegal, p["collision_reward"], 0.0)) * p["reward_scale"]
    return r, (bool(p["done_at_collision"]) & illegal) | (bool(p["done_at_success"]) & (dist <= p["goal_dist"]))


def scripted_steps(n, steps, horizon, seed, p_done=0.3):
    """Synthetic step outputs of n envs: random rows, a done pattern of early ends and timeouts (no episode longer than `horizon`), collision types of
    every class.  Yields (actions f64 [n, 7], obs, term_obs f32 [n, 64], reward f32 [n], done u8 [n], info i32 [n, 14])."""
    rng = np.random.RandomState(seed)
    age = np.zeros(n, np.int64)
    for _ in range(steps):
        age += 1
        timeout = age >= horizon
        done = timeout | (rng.uniform(size=n) < p_done)
        info = np.zeros((n, INFO_DIM), np.int32)
        info[:, INFO_TRUNCATED] = timeout & (rng.uniform(size=n) < 0.8)   # (a timeout step on which the env itself finished is no truncation)
        info[:, INFO_COLLISION_TYPE] = rng.choice([0, 1, 2, 4, 8, 16], size=n)
        obs, term = rng.uniform(-1, 1, (n, 64)).astype(np.float32), rng.uniform(-1, 1, (n, 64)).astype(np.float32)
        obs[:, 39], term[:, 39] = rng.randint(0, 2, n), rng.randint(0, 2, n)   # object_gripped: a flag
        yield rng.uniform(-1.5, 1.5, (n, 7)), obs, term, rng.uniform(-2, 2, n).astype(np.float32), done.astype(np.uint8), info
        age[done] = 0


class Ring:
    """The rings of n envs: the arrays of hrg_her_export, [n, cap, ...] / [n]."""

    def __init__(self, n, cap, act_dim=7, act_bounds=None):
        self.n, self.cap, self.act_dim, self.act_bounds = n, cap, act_dim, act_bounds
        self.pre, self.post = np.zeros((n, cap, OBS_DIM), np.float32), np.zeros((n, cap, OBS_DIM), np.float32)
        self.action, self.reward = np.zeros((n, cap, act_dim), np.float32), np.zeros((n, cap), np.float32)
        self.done, self.truncated, self.collision_type = np.zeros((n, cap), np.uint8), np.zeros((n, cap), np.uint8), np.zeros((n, cap), np.int32)
        self.ep_start, self.ep_len = np.zeros((n, cap), np.int64), np.zeros((n, cap), np.int32)
        self.w, self.tail, self.open = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.cur_obs = np.zeros((n, OBS_DIM), np.float32)

    def observe(self, obs, mask=None):
        for e in range(self.n):
            if mask is None or mask[e]:
                self.cur_obs[e] = obs[e]
                self.w[e] = self.open[e]

    def add(self, actions, obs, term_obs, reward, done, info):
        cap = self.cap
        for e in range(self.n):
            w, tail, opn = int(self.w[e]), int(self.tail[e]), int(self.open[e])
            if w - tail == cap:   # the oldest episode leaves whole
                ts = tail % cap
                assert self.ep_len[e, ts] > 0, "an episode longer than the ring"
                tail = int(self.ep_start[e, ts]) + int(self.ep_len[e, ts])
            s = w % cap
            self.pre[e, s] = self.cur_obs[e]
            self.post[e, s] = term_obs[e] if done[e] else obs[e]
            self.cur_obs[e] = obs[e]
            a = np.asarray(actions[e, :self.act_dim], np.float64)
            if self.act_bounds is not None:   # HER_buffer_add_monkey_patch.py:64-76
                low, high = (np.asarray(b, np.float64)[:self.act_dim] for b in self.act_bounds)
                a = np.clip(2.0 * ((a - low) / (high - low)) - 1.0, -1, 1)
            self.action[e, s] = a.astype(np.float32)
            self.reward[e, s], self.done[e, s] = reward[e], 1 if done[e] else 0
            self.truncated[e, s], self.collision_type[e, s] = int(info[e, INFO_TRUNCATED] != 0), info[e, INFO_COLLISION_TYPE]
            self.ep_start[e, s], self.ep_len[e, s] = opn, 0
            w += 1
            if done[e]:
                L = w - opn
                for k in range(L):
                    self.ep_len[e, (opn + k) % cap] = L
                opn = w
            self.w[e], self.tail[e], self.open[e] = w, tail, opn

    def counts(self):
        return self.open - self.tail

    def export(self, e):
        d = {k: getattr(self, k)[e] for k in ("pre", "post", "action", "reward", "done", "truncated", "collision_type", "ep_start", "ep_len", "cur_obs")}
        d.update(w=int(self.w[e]), tail=int(self.tail[e]), open=int(self.open[e]))
        return d


def sample(ring, u01, seed, call, batch, kind, ratio, strategy="future", params=PARAMS, obs_cols=range(OBS_DIM), relabel_observation=False, dg_in_obs=()):
    """The sample kernel's batch: dict of index [B, 3] (env, counter, goal counter or -1), t, L, f, relabel, the nine outputs, and `margin` = | distance -
    goal_dist | of the relabelled samples (inf elsewhere)."""
    counts = ring.counts()
    cum = np.concatenate([[0], np.cumsum(counts)])
    N, cap = int(cum[-1]), ring.cap
    assert N > 0
    cols, ag_c, dg_c, ng_c = list(obs_cols), AG_COLS[kind], DG_COLS[kind], NEW_GOAL_COLS[kind]
    out = dict(index=np.zeros((batch, 3), np.int64), t=np.zeros(batch, np.int64), L=np.zeros(batch, np.int64), f=np.zeros(batch, np.int64), relabel=np.zeros(batch, bool),
               observation=np.zeros((batch, len(cols)), np.float32), next_observation=np.zeros((batch, len(cols)), np.float32),
               achieved_goal=np.zeros((batch, len(ag_c)), np.float32), next_achieved_goal=np.zeros((batch, len(ag_c)), np.float32),
               desired_goal=np.zeros((batch, len(dg_c)), np.float32), action=np.zeros((batch, ring.act_dim), np.float32), reward=np.zeros((batch, 1), np.float64),
               done=np.zeros((batch, 1), np.float32), margin=np.full(batch, np.inf))
    for k in range(batch):
        u = [u01(seed, call, k, STREAM_HER, d) for d in range(3)]
        j = min(int(np.floor(u[0] * N)), N - 1)
        e = int(np.searchsorted(cum, j, side="right")) - 1
        i = int(ring.tail[e]) + (j - int(cum[e]))
        s = i % cap
        es, L = int(ring.ep_start[e, s]), int(ring.ep_len[e, s])
        t = i - es
        relabel = u[1] < ratio
        if strategy == "future":
            f = t + min(int(np.floor(u[2] * (L - t))), L - t - 1)
        elif strategy == "final":
            f = L - 1
        else:
            f = min(int(np.floor(u[2] * L)), L - 1)
        pre, post = ring.pre[e, s], ring.post[e, s]
        goal, rew, dn = pre[dg_c], float(ring.reward[e, s]), bool(ring.done[e, s]) and not ring.truncated[e, s]
        ob, nob = pre[cols].copy(), post[cols].copy()
        if relabel:
            goal = ring.post[e, (es + f) % cap][ng_c]
            r, d = reward_done(kind, params, post[ag_c], goal, ring.collision_type[e, s])
            rew, dn = float(r[0]), bool(d[0])
            out["margin"][k] = abs(float(goal_distance(kind, post[ag_c], goal)[0]) - params["goal_dist"])
            if relabel_observation:
                ob[list(dg_in_obs)] = goal
                nob[list(dg_in_obs)] = goal
        out["index"][k] = (e, i, es + f if relabel else -1)
        out["t"][k], out["L"][k], out["f"][k], out["relabel"][k] = t, L, f, relabel
        out["observation"][k], out["next_observation"][k] = ob, nob
        out["achieved_goal"][k], out["next_achieved_goal"][k], out["desired_goal"][k] = pre[ag_c], post[ag_c], goal
        out["action"][k], out["reward"][k, 0], out["done"][k, 0] = ring.action[e, s], rew, float(dn)
    out["next_desired_goal"] = out["desired_goal"]
    return out
