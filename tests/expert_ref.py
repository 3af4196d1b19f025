"""numpy restatement of the scripted experts, their Ornstein-Uhlenbeck noise, the similarity functions and the reward mix of the action-based
expert imitation reward -- what csrc/hrgym_expert.h computes, row-vectorised, FP64.  Written from the behaviour (like hullbox_ref.py); the recorded
outputs of the reference's own expert classes are tests/golden/expert_ref.npz (tools/make_expert_fixtures.py), which test_expert.py holds this file to.

Every function takes arrays with a leading row axis.  `noise` is the noise process's state AFTER this call's step ([n, 3], or [n, 7] for the reach
expert), or None for signal_to_noise_ratio = 1, where it cannot show.
"""
import numpy as np

TAN_HALF = float(np.tan(0.5))
STREAM_EXPERT = 8
# columns of the 64-wide observation superset the experts read (vec_env.OBS_COLUMNS / OBS_COLUMNS_TASK)
COLS = dict(goal_difference=slice(12, 18), object_gripped=39, vec_eef_to_object=slice(40, 43), vec_eef_to_target=slice(43, 46), robot0_gripper_qpos=slice(53, 55),
            vec_eef_to_human_lh=slice(0, 3), vec_eef_to_human_rh=slice(4, 7), vec_eef_to_nail=slice(43, 46))
PICK_PLACE_DEFAULTS = dict(hover_dist=0.2, tan_theta=0.5, horizontal_epsilon=0.03, vertical_epsilon=0.015, goal_dist=0.08, gripper_fully_opened_threshold=0.02,
                           release_when_delivered=True)
OU_PARAMS = {"ReachHuman": (10.0, 0.5)}   # (alpha, sigma); the Cartesian experts: (0.5, motion limit / 2)


def _zero(noise, n, dim):
    return np.zeros((n, dim)) if noise is None else np.asarray(noise, np.float64)


def reach(goal_difference, low, high, snr=1.0, noise=None):
    """[n, 6] -> [n, 7]: the joint deltas to the goal, gripper 0; noise scaled to half the action range; clipped before and after the mix."""
    gd = np.asarray(goal_difference, np.float64)
    low, high = np.asarray(low, np.float64), np.asarray(high, np.float64)
    motion = np.clip(np.concatenate([gd, np.zeros((len(gd), 1))], axis=1), low, high)
    return np.clip(snr * motion + _zero(noise, len(gd), 7) * (1 - snr) * 0.5 * (high - low), low, high)


def pick_place_predicates(gripped, to_obj, to_tgt, qpos, horizontal_epsilon=0.03, vertical_epsilon=0.015, tan_theta=0.5, gripper_fully_opened_threshold=0.02, **_):
    """The expert's six predicates and, for each, its margin: the distance of the deciding quantity from its threshold (min over a conjunction's terms)."""
    o, t = np.asarray(to_obj, np.float64), np.asarray(to_tgt, np.float64)
    q = np.asarray(qpos, np.float64)
    he, ve = horizontal_epsilon, vertical_epsilon
    o2t = t - o
    terms = dict(
        opened=[(q[:, 0] - q[:, 1]) - gripper_fully_opened_threshold],
        delivered=[he - np.hypot(o2t[:, 0], o2t[:, 1]), ve - np.abs(o2t[:, 2])],
        at_object=[he - np.hypot(o[:, 0], o[:, 1]), ve + o[:, 2]],
        above_object=[(he - o[:, 2] * tan_theta) - np.hypot(o[:, 0], o[:, 1]), -o[:, 2]],
        above_target=[(he - t[:, 2] * tan_theta) - np.hypot(t[:, 0], t[:, 1]), -t[:, 2]],
    )
    pred = {k: np.all([m > 0 for m in v], axis=0) for k, v in terms.items()}
    pred["gripped"] = np.asarray(gripped).astype(bool)
    margin = np.min([np.abs(m) for v in terms.values() for m in v], axis=0)
    return pred, margin


def pick_place_branches(pred, release_when_delivered=True):
    """(motion branch 0..4, gripper branch 0..2) in the expert's order of tests: above the object after delivery | down to the object | down to the
    target | above the target | above the object;  open after delivery | close (gripped or at the object) | open."""
    p = pred
    motion = np.select([p["delivered"] & p["opened"], p["above_object"] & p["opened"], p["above_target"] & p["gripped"], p["gripped"]], [0, 1, 2, 3], 4)
    grip = np.select([p["delivered"] & bool(release_when_delivered), p["gripped"] | p["at_object"]], [0, 1], 2)
    return motion, grip


def pick_place(gripped, to_obj, to_tgt, qpos, lim, glim=1.0, snr=1.0, noise=None, **params):
    """-> [n, 4]: hover above / descend to the object or the target, gripper open (-1) / closed (+1).  The noise enters the motion only."""
    kw = dict(PICK_PLACE_DEFAULTS, **params)
    o, t = np.asarray(to_obj, np.float64), np.asarray(to_tgt, np.float64)
    pred, _ = pick_place_predicates(gripped, o, t, qpos, **kw)
    mb, gb = pick_place_branches(pred, kw["release_when_delivered"])
    motion = np.where(((mb == 2) | (mb == 3))[:, None], t, o).copy()
    motion[:, 2] += np.where((mb == 0) | (mb == 3) | (mb == 4), kw["hover_dist"], 0.0)
    motion = np.clip(motion, -lim, lim)
    motion = np.clip(motion * snr + _zero(noise, len(o), 3) * (1 - snr), -lim, lim)
    g = np.clip(np.where(gb == 1, 1.0, -1.0), -glim, glim)
    return np.concatenate([motion, g[:, None]], axis=1)


def lifting(to_lh, to_rh, lim, glim=1.0, board_size=(1.0, 0.4, 0.03), human_grip_offset=0.1, snr=1.0, noise=None):
    """-> [n, 4]: to the height of the midpoint of the human's hands, a board length minus the grip offset away from it; gripper closed.  Motion and
    noise are clipped, their mix is not."""
    v = (np.asarray(to_lh, np.float64) + np.asarray(to_rh, np.float64)) / 2
    flat = v[:, :2] / np.linalg.norm(v, axis=1)[:, None]
    motion = np.clip(np.concatenate([v[:, :2] - (board_size[0] - human_grip_offset) * flat, v[:, 2:3]], axis=1), -lim, lim)
    act = motion * snr + np.clip(_zero(noise, len(v), 3), -lim, lim) * (1 - snr)
    return np.concatenate([act, np.full((len(v), 1), float(glim))], axis=1)


def hammering(to_nail):
    """-> [n, 4]: to a point 0.1 in front of the nail (-x), clipped to 0.1; gripper closed; no noise."""
    v = np.asarray(to_nail, np.float64)
    return np.concatenate([np.clip(v + np.array([-0.1, 0.0, 0.0]), -0.1, 0.1), np.ones((len(v), 1))], axis=1)


def expert_from_obs(expert_id, full, low, high, snr=1.0, noise=None, **params):
    """The expert's action on rows of the 64-wide observation superset (bounds of the env's action space: length 4 or 7)."""
    f = np.asarray(full, np.float64)
    low, high = np.asarray(low, np.float64), np.asarray(high, np.float64)
    if expert_id == "ReachHuman":
        return reach(f[:, COLS["goal_difference"]], low, high, snr, noise)
    if expert_id == "PickPlaceHumanCart":
        return pick_place(f[:, COLS["object_gripped"]] != 0, f[:, COLS["vec_eef_to_object"]], f[:, COLS["vec_eef_to_target"]], f[:, COLS["robot0_gripper_qpos"]],
                          high[0], high[3], snr, noise, **params)
    if expert_id == "CollaborativeLiftingCart":
        return lifting(f[:, COLS["vec_eef_to_human_lh"]], f[:, COLS["vec_eef_to_human_rh"]], high[0], high[3], snr=snr, noise=noise, **params)
    if expert_id == "CollaborativeHammeringCart":
        return hammering(f[:, COLS["vec_eef_to_nail"]])
    raise KeyError(expert_id)


def ou_params(expert_id, lim):
    """(alpha, sigma, dim) of the expert's noise process."""
    return (10.0, 0.5, 7) if expert_id == "ReachHuman" else (0.5, 0.5 * lim, 3)


def ou_step(y, xi, alpha, sigma, dt, mu=0.0):
    """y <- y + alpha (mu - y) dt + sigma sqrt(2 alpha) sqrt(dt) xi"""
    return y + (alpha * (mu - y) * dt + sigma * np.sqrt(2 * alpha) * np.sqrt(dt) * xi)


def ou_stationary_variance(alpha, sigma, dt):
    """Variance the Euler-Maruyama recursion settles at: y' = (1 - alpha dt) y + b xi has var = b^2 / (1 - (1 - alpha dt)^2) = sigma^2 / (1 - alpha dt / 2)."""
    return sigma * sigma / (1 - alpha * dt / 2)


def gauss(u01, seed, gid, call, dim):
    """The `dim` standard normals of noise step number `call` of global env `gid`: Box-Muller over the counter hash u01(seed, env, episode, stream, idx)
    (the oracle's hrgo_test_u01), keyed by (seed, gid, 0, STREAM_EXPERT, 2 (call dim + k) [+ 1])."""
    out = np.empty(dim)
    for k in range(dim):
        i = call * dim + k
        u1, u2 = u01(seed, gid, 0, STREAM_EXPERT, 2 * i), u01(seed, gid, 0, STREAM_EXPERT, 2 * i + 1)
        out[k] = np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)
    return out


def similarity(name, delta, iota):
    delta = np.asarray(delta, np.float64)
    if name == "gaussian":
        return 2.0 ** (-(delta / iota) ** 2)
    if name == "tanh":
        return -np.tanh(TAN_HALF * delta / iota) + 1
    raise ValueError(f"Unknown similarity function: {name}")


def imitation_reward(agent, expert, beta, iota_m, iota_g, m_sim_fn="gaussian", g_sim_fn="gaussian", normalize_joint_actions=False, low=None, high=None):
    """(r_im, r_motion, r_gripper) for action rows of width 4 (Cartesian: distance over [:3], |[3]|) or 7 (joint: distance over [:6], |[6]|)."""
    a, x = np.asarray(agent, np.float64), np.asarray(expert, np.float64)
    am, xm = a[:, :-1], x[:, :-1]
    if a.shape[1] == 7 and normalize_joint_actions:
        lo, hi = np.asarray(low, np.float64)[:-1], np.asarray(high, np.float64)[:-1]
        am, xm = 2 * (am - lo) / (hi - lo) - 1, 2 * (xm - lo) / (hi - lo) - 1
    r_m = similarity(m_sim_fn, np.linalg.norm(am - xm, axis=1), iota_m)
    r_g = similarity(g_sim_fn, np.abs(a[:, -1] - x[:, -1]), iota_g)
    return r_m * beta + r_g * (1 - beta), r_m, r_g


def combine(r_im, r_env, alpha):
    return r_im * alpha + r_env * (1 - alpha)
