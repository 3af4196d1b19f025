"""Scripted experts and the action-based expert imitation reward, as keyword dicts -> `hrg_expert_desc` (include/hrgym.h).

`expert` is the reference's `config.expert` node as `create_expert` consumes it (utils/training_utils.py:138-174): `id` selects the class of
demonstrations/experts/ (REGISTERED_EXPERTS), `obs_keys` is dropped, everything else is a constructor argument.  `imitation_reward` is
`config.wrappers.action_based_expert_imitation_reward` without `rsi_prob` / `dataset_name` (training_utils.py:252-271).  The kernels are in
csrc/hrgym_expert.h.
"""
import numpy as np

from ._cstruct import CONST, ExpertDesc
from .tasks import TASKS

# REGISTERED_EXPERTS (demonstrations/experts/__init__.py:8-14) -> HRG_EXPERT_*
EXPERT_IDS = {"ReachHuman": CONST["HRG_EXPERT_REACH"], "PickPlaceHumanCart": CONST["HRG_EXPERT_PICK_PLACE"],
              "CollaborativeLiftingCart": CONST["HRG_EXPERT_LIFTING"], "CollaborativeHammeringCart": CONST["HRG_EXPERT_HAMMERING"],
              "ReachHumanCart": CONST["HRG_EXPERT_REACH_CART"]}
_REQUIRED = object()
# constructor arguments and their defaults, per expert class
EXPERT_KWARGS = {
    "ReachHuman": dict(signal_to_noise_ratio=1.0, delta_time=0.01, seed=None),
    "PickPlaceHumanCart": dict(signal_to_noise_ratio=1.0, hover_dist=0.2, tan_theta=0.5, horizontal_epsilon=0.03, vertical_epsilon=0.015, goal_dist=0.08,
                               gripper_fully_opened_threshold=0.02, release_when_delivered=True, delta_time=0.01, seed=None),
    "CollaborativeLiftingCart": dict(signal_to_noise_ratio=_REQUIRED, board_size=_REQUIRED, human_grip_offset=0.1, delta_time=0.01, seed=None),
    "CollaborativeHammeringCart": dict(signal_to_noise_ratio=1.0, delta_time=0.1, seed=None),
    "ReachHumanCart": dict(signal_to_noise_ratio=1.0, delta_time=0.01, seed=None),
}
EXPERT_ENVS = {eid: tuple(env_id for env_id, t in TASKS.items() if eid in t.experts) for eid in EXPERT_KWARGS}   # the tasks whose observation an expert reads
SIM_FNS = {"gaussian": CONST["HRG_SIM_GAUSSIAN"], "tanh": CONST["HRG_SIM_TANH"]}
IMITATION_REWARD_KWARGS = dict(alpha=0.0, beta=0.0, iota_m=0.1, iota_g=0.25, m_sim_fn="gaussian", g_sim_fn="gaussian", normalize_joint_actions=False)   # the last: Joint form only
IMIT_COLUMNS = ("r_im", "r_env", "r_motion", "r_gripper", "ep_im", "ep_env", "ep_len", "r_full")   # HRG_IMIT_*


def expert_kwargs(expert):
    """`expert` dict -> (id, constructor kwargs with the defaults filled in).  Unknown ids / arguments raise."""
    kw = dict(expert)
    eid = kw.pop("id", None)
    kw.pop("obs_keys", None)
    if eid not in EXPERT_KWARGS:
        raise NotImplementedError(f"expert id {eid!r}: available {sorted(EXPERT_KWARGS)}")
    known = EXPERT_KWARGS[eid]
    unknown = sorted(set(kw) - set(known))
    if unknown:
        raise TypeError(f"expert {eid}: unexpected arguments {unknown} (its constructor takes {sorted(known)})")
    out = {k: kw.get(k, v) for k, v in known.items()}
    missing = sorted(k for k, v in out.items() if v is _REQUIRED)
    if missing:
        raise TypeError(f"expert {eid}: missing required arguments {missing}")
    return eid, out


def imitation_reward_kwargs(imitation_reward, cartesian=False):
    kw = dict(imitation_reward)
    unknown = sorted(set(kw) - set(IMITATION_REWARD_KWARGS) | ({"normalize_joint_actions"} & set(kw) if cartesian else set()))   # the Cart wrapper has no such argument
    if unknown:
        raise TypeError(f"imitation_reward: unexpected arguments {unknown} (the wrapper takes {sorted(IMITATION_REWARD_KWARGS)})")
    out = {k: kw.get(k, v) for k, v in IMITATION_REWARD_KWARGS.items()}
    for k in ("m_sim_fn", "g_sim_fn"):
        if out[k] not in SIM_FNS:
            raise ValueError(f"Unknown similarity function: {out[k]}")
    return out


def build_expert_desc(expert, act_low, act_high, imitation_reward=None, default_seed=0):
    """hrg_expert_desc of `expert` (+ `imitation_reward`) for an action space with bounds act_low / act_high (length 4: Cartesian, length 7: joint).
    `seed: None` in the reference seeds the noise from the operating system's entropy; here it falls back to `default_seed` (HipVecEnv: the env seed)."""
    eid, kw = expert_kwargs(expert)
    lo, hi = np.asarray(act_low, np.float64).ravel(), np.asarray(act_high, np.float64).ravel()
    if lo.shape != hi.shape or lo.shape[0] not in (4, CONST["HRG_ACT_DIM"]):
        raise ValueError(f"action bounds of length {lo.shape[0]}: expected 4 (Cartesian) or {CONST['HRG_ACT_DIM']} (joint)")
    d = ExpertDesc()
    d.expert = EXPERT_IDS[eid]
    d.cartesian = int(lo.shape[0] == 4)
    for k in range(lo.shape[0]):
        d.act_low[k], d.act_high[k] = float(lo[k]), float(hi[k])
    d.signal_to_noise_ratio = float(kw["signal_to_noise_ratio"])
    d.delta_time = float(kw["delta_time"])
    d.seed = int(default_seed if kw["seed"] is None else kw["seed"]) & 0xFFFFFFFFFFFFFFFF
    if eid == "PickPlaceHumanCart":   # (goal_dist: a constructor argument the reference's expert stores and never reads; carried, unused by the kernel)
        for k in ("hover_dist", "tan_theta", "horizontal_epsilon", "vertical_epsilon", "goal_dist", "gripper_fully_opened_threshold"):
            setattr(d, k, float(kw[k]))
        d.release_when_delivered = int(bool(kw["release_when_delivered"]))
    if eid == "CollaborativeLiftingCart":
        bs = np.asarray(kw["board_size"], np.float64).ravel()
        if bs.shape != (3,):
            raise ValueError("expert CollaborativeLiftingCart: board_size must be [x, y, z]")
        for k in range(3):
            d.board_size[k] = float(bs[k])
        d.human_grip_offset = float(kw["human_grip_offset"])
    if imitation_reward is not None:
        r = imitation_reward_kwargs(imitation_reward, cartesian=bool(d.cartesian))
        d.reward_enabled = 1
        d.alpha, d.beta, d.iota_m, d.iota_g = float(r["alpha"]), float(r["beta"]), float(r["iota_m"]), float(r["iota_g"])
        d.m_sim_fn, d.g_sim_fn = SIM_FNS[r["m_sim_fn"]], SIM_FNS[r["g_sim_fn"]]
        d.normalize_joint_actions = int(bool(r["normalize_joint_actions"]))
    return d
