"""numpy restatement of the three state-based expert imitation rewards (wrappers/state_based_expert_imitation_reward_wrapper.py: ReachHuman 361-413,
PickPlaceHumanCart 542-619, CollaborativeLiftingCart 698-758), of DatasetRSIWrapper's cursor (wrappers/dataset_wrapper.py:115-157) and of the restore
kernel's three draws.  FP64 on rows of the 64-column observation superset, vectorised over envs; checked against the reference's recorded outputs
(tests/golden/sir_ref.npz) in tests/test_dataset.py and used as the device's reference in tests/test_dataset_gpu.py."""
import numpy as np

from expert_ref import similarity   # utils/expert_imitation_reward_utils.py:51-73, restated once

KINDS = ("reach", "pick_place", "lifting")           # HRG_SIR_REACH, _PICK_PLACE, _LIFTING = 1, 2, 3
# columns of vec_env.OBS_COLUMNS
GOAL_DIFF, GRIPPED, TO_TARGET, GRIPPER_QPOS, TO_HUMAN_LH = slice(12, 18), 39, slice(43, 46), slice(53, 55), slice(0, 3)
STREAM_DATASET = 9


def distance(kind, demo, policy):
    """||demonstration - policy|| of the columns the wrapper of `kind` compares."""
    cols = GOAL_DIFF if kind == "reach" else TO_TARGET if kind == "pick_place" else TO_HUMAN_LH
    d = np.asarray(demo, np.float64)[:, cols] - np.asarray(policy, np.float64)[:, cols]
    return np.array([np.linalg.norm(r) for r in d])   # row by row, as the wrappers call it: the 1-D norm is sqrt(dot(x, x)), whose sum need not round like add.reduce's


def mismatch(kind, demo, policy):
    """The demonstration has gripped and the agent has not (never for ReachHuman)."""
    if kind == "reach":
        return np.zeros(len(demo), bool)
    return (np.asarray(demo)[:, GRIPPED] != 0) & ~(np.asarray(policy)[:, GRIPPED] != 0)


def imitation_reward(kind, demo, policy, beta=1.0, iota_m=0.1, iota_g=0.05, m_sim_fn="gaussian", g_sim_fn="gaussian"):
    """_get_imitation_reward: (r_im, r_motion, r_gripper, counted).  r_motion / r_gripper are pick-place's two terms (zero elsewhere, and zero with
    `counted` False on a gripped-mismatch step, which the wrapper does not append to its motion / gripper lists)."""
    demo, policy = np.asarray(demo, np.float64), np.asarray(policy, np.float64)
    dist, mm = distance(kind, demo, policy), mismatch(kind, demo, policy)
    zero = np.zeros(len(demo))
    if kind == "pick_place":
        g = demo[:, GRIPPER_QPOS] - policy[:, GRIPPER_QPOS]
        r_m = similarity(m_sim_fn, dist, iota_m)
        r_g = similarity(g_sim_fn, np.abs(g[:, 0] - g[:, 1]), iota_g)
        r_im = r_m * beta + r_g * (1 - beta)
        return np.where(mm, 0.0, r_im), np.where(mm, 0.0, r_m), np.where(mm, 0.0, r_g), ~mm
    r = similarity(m_sim_fn, dist, iota_m)
    return np.where(mm, 0.0, r), zero, zero, np.zeros(len(demo), bool)


def et_margin(kind, demo, policy, iota_m=0.1, et_dist=2.0):
    """|distance - threshold| to the nearest early-termination threshold that decides the env's verdict."""
    dist, mm = distance(kind, demo, policy), mismatch(kind, demo, policy)
    m = np.abs(dist - et_dist * iota_m)
    if kind == "pick_place":
        m = np.where(mm, np.minimum(m, np.abs(dist - et_dist * 0.1 * iota_m)), m)
    return m


def early_termination(kind, demo, policy, iota_m=0.1, et_dist=2.0):
    """_should_terminate_early."""
    dist, mm = distance(kind, demo, policy), mismatch(kind, demo, policy)
    if kind == "reach":
        return dist > et_dist * iota_m
    if kind == "pick_place":
        return (mm & (dist > et_dist * 0.1 * iota_m)) | (dist > et_dist * iota_m)
    return mm | (dist > et_dist * iota_m)


def combine(r_im, r_env, alpha):
    return r_im * alpha + r_env * (1 - alpha)


def advance(step, T):
    """DatasetRSIWrapper.step (149)."""
    return np.minimum(np.asarray(step) + 1, np.asarray(T))


def draw_cursor(u01, seed, gid, n_resets, ep_offset, rsi_prob):
    """The restore kernel's (episode, start step, T) of global env `gid` at its `n_resets`-th restore, over the counter hash u01(seed, env, episode, stream,
    idx) (the oracle's hrgo_test_u01), keyed by (dataset seed, gid, n_resets, STREAM_DATASET, 0..2)."""
    n_ep = len(ep_offset) - 1
    u = [u01(seed, gid, n_resets, STREAM_DATASET, k) for k in range(3)]
    ep = min(int(np.floor(u[0] * n_ep)), n_ep - 1)
    T = int(ep_offset[ep + 1] - ep_offset[ep])
    step = min(int(np.floor(u[2] * T)), T - 1) if u[1] < rsi_prob else 0
    return ep, step, T
