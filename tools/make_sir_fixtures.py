#!/usr/bin/env python3
"""Record what the reference's state-based expert imitation reward wrappers compute: python tools/make_sir_fixtures.py REFERENCE_CHECKOUT [OUT.npz]

Loads the reference's own wrappers/state_based_expert_imitation_reward_wrapper.py, builds its three wrapper classes without their constructors
(object.__new__ + their private parameters: the constructors load a dataset from disk and wrap a gym env) and calls `_get_imitation_reward` and
`_should_terminate_early` on random f32-representable expert observation dicts.  Writes tests/golden/sir_ref.npz: inputs (as rows of the 64-column
observation superset), parameters, outputs.  Build machine only: no test reads the checkout.

Stand-ins (recorded in the file's `note`): bare package shells for `human_robot_gym`, `.utils`, `.demonstrations`, `.wrappers` (their __init__ files are
not executed; the modules below them load from the checkout unchanged); `gym` = {Space, Env, Wrapper, core.Env, spaces.Box(low, high)};
`robosuite.environments.MujocoEnv`, `robosuite.wrappers.{Wrapper, GymWrapper}` as empty classes; `human_robot_gym.utils.mjcf_utils.file_path_completion`
as the identity.  pandas (imported by wrappers/dataset_wrapper.py) is the installed one.
"""
import os
import sys
import types

import numpy as np

ROWS = 321          # one full 256-thread block + 65
POOL = 480
MARGIN = 1e-9       # rows whose distance lies this close to an early-termination threshold are dropped
MIN_PER_GROUP = 20  # rows that must survive per (gripped-mismatch branch, verdict)
PARAMS = dict(reach=dict(iota=0.1, et_dist=2.0), pick_place=dict(beta=0.7, iota_m=0.1, iota_g=0.05, et_dist=2.0), lifting=dict(iota=0.15, et_dist=1.5))
SIM_FNS = ("gaussian", "tanh")


def install_stand_ins(ref):
    gym, spaces, core = types.ModuleType("gym"), types.ModuleType("gym.spaces"), types.ModuleType("gym.core")

    class Space:
        pass

    class Box(Space):
        def __init__(self, low, high, dtype=np.float64):
            self.low, self.high = np.asarray(low, dtype), np.asarray(high, dtype)
            self.shape = self.low.shape

    class Env:
        pass

    class Wrapper(Env):
        pass

    gym.Space, gym.Env, gym.Wrapper, gym.spaces, gym.core, spaces.Box, core.Env = Space, Env, Wrapper, spaces, core, Box, Env
    sys.modules.update({"gym": gym, "gym.spaces": spaces, "gym.core": core})
    rs, rse, rsw = types.ModuleType("robosuite"), types.ModuleType("robosuite.environments"), types.ModuleType("robosuite.wrappers")
    rse.MujocoEnv, rsw.Wrapper, rsw.GymWrapper = type("MujocoEnv", (), {}), type("Wrapper", (), {}), type("GymWrapper", (), {})
    rs.environments, rs.wrappers = rse, rsw
    sys.modules.update({"robosuite": rs, "robosuite.environments": rse, "robosuite.wrappers": rsw})
    root = os.path.join(ref, "human_robot_gym")
    for name, sub in (("human_robot_gym", ""), ("human_robot_gym.utils", "utils"), ("human_robot_gym.demonstrations", "demonstrations"),
                      ("human_robot_gym.wrappers", "wrappers")):
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(root, sub)]
        sys.modules[name] = m
    mj = types.ModuleType("human_robot_gym.utils.mjcf_utils")
    mj.file_path_completion = lambda p: p
    sys.modules["human_robot_gym.utils.mjcf_utils"] = mj


def f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def main():
    ref = os.path.abspath(sys.argv[1])
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(here, "tests", "golden", "sir_ref.npz")
    sys.path.insert(0, os.path.join(here, "tests"))
    import sir_ref as R   # distances to the thresholds (which rows to drop); the recorded outputs below are the reference's alone
    install_stand_ins(ref)
    from human_robot_gym.wrappers import state_based_expert_imitation_reward_wrapper as W
    rng = np.random.RandomState(20241)
    classes = dict(reach=W.ReachHumanStateBasedExpertImitationRewardWrapper, pick_place=W.PickPlaceHumanCartStateBasedExpertImitationRewardWrapper,
                   lifting=W.CollaborativeLiftingCartStateBasedExpertImitationRewardWrapper)
    data = {}
    for kind in R.KINDS:
        p = PARAMS[kind]
        iota_m = p.get("iota", p.get("iota_m"))
        width = 6 if kind == "reach" else 3
        # demonstration and agent vectors a multiple of iota apart, spread over both sides of the thresholds (et_dist iota; 0.1 of it for pick-place)
        base = rng.uniform(-0.5, 0.5, (POOL, width))
        dirs = rng.normal(size=(POOL, width))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        sep = iota_m * rng.choice([0.02, 0.1, 0.15, 0.3, 1.0, 1.8, 2.5, 4.0], POOL) * rng.uniform(0.5, 1.5, POOL)
        demo, pol = np.zeros((POOL, 64), np.float32), np.zeros((POOL, 64), np.float32)
        cols = R.GOAL_DIFF if kind == "reach" else R.TO_TARGET if kind == "pick_place" else R.TO_HUMAN_LH
        demo[:, cols], pol[:, cols] = base, base + dirs * sep[:, None]
        if kind != "reach":
            demo[:, R.GRIPPED], pol[:, R.GRIPPED] = rng.rand(POOL) < 0.5, rng.rand(POOL) < 0.5
        if kind == "pick_place":
            for rows in (demo, pol):
                rows[:, R.GRIPPER_QPOS] = np.stack([rng.uniform(0, 0.021, POOL), -rng.uniform(0, 0.021, POOL)], axis=1)
                rows[:, 40:43] = rng.uniform(-0.3, 0.3, (POOL, 3))      # vec_eef_to_object: read into the expert observation, not compared
        if kind == "lifting":
            for rows in (demo, pol):
                rows[:, 4:7] = rng.uniform(-0.5, 0.5, (POOL, 3))        # vec_eef_to_human_rh: likewise
        keep = R.et_margin(kind, demo, pol, iota_m=iota_m, et_dist=p["et_dist"]) >= MARGIN
        idx = np.nonzero(keep)[0][:ROWS]
        assert len(idx) == ROWS, f"{kind}: {keep.sum()} of {POOL} rows survive"
        demo, pol = demo[idx], pol[idx]

        def obs_dict(row):
            row = row.astype(np.float64)
            if kind == "reach":
                return dict(goal_difference=row[R.GOAL_DIFF])
            if kind == "pick_place":
                return dict(object_gripped=bool(row[R.GRIPPED]), vec_eef_to_object=row[40:43], vec_eef_to_target=row[R.TO_TARGET], robot0_gripper_qpos=row[R.GRIPPER_QPOS])
            return dict(vec_eef_to_human_lh=row[R.TO_HUMAN_LH], vec_eef_to_human_rh=row[4:7], board_quat=np.array([0.0, 0.0, 0.0, 1.0]), board_gripped=bool(row[R.GRIPPED]))

        data[kind + "_demo"], data[kind + "_policy"] = demo, pol
        for fn in SIM_FNS:
            w = object.__new__(classes[kind])
            w._alpha, w._et_dist = 0.5, p["et_dist"]
            if kind == "pick_place":
                w._beta, w._iota_m, w._iota_g, w._m_sim_fn, w._g_sim_fn = p["beta"], p["iota_m"], p["iota_g"], fn, SIM_FNS[1 - SIM_FNS.index(fn)]
            else:
                w._iota, w._sim_fn = p["iota"], fn
            r_im, et, r_m, r_g = np.zeros(ROWS), np.zeros(ROWS, bool), np.full(ROWS, np.nan), np.full(ROWS, np.nan)
            for i in range(ROWS):
                w._motion_imitation_rewards, w._gripper_imitation_rewards = [], []
                d, q = obs_dict(demo[i]), obs_dict(pol[i])
                r_im[i] = w._get_imitation_reward(demonstration_obs_dict=d, policy_obs_dict=q)
                et[i] = bool(w._should_terminate_early(demonstration_obs_dict=d, policy_obs_dict=q))
                if w._motion_imitation_rewards:    # pick-place appends its two terms unless the demonstration has gripped and the agent has not
                    r_m[i], r_g[i] = w._motion_imitation_rewards[0], w._gripper_imitation_rewards[0]
            data[f"{kind}_{fn}_r_im"], data[f"{kind}_{fn}_et"], data[f"{kind}_{fn}_r_motion"], data[f"{kind}_{fn}_r_gripper"] = r_im, et, r_m, r_g
        mm, et = R.mismatch(kind, demo, pol), data[f"{kind}_gaussian_et"]
        groups = [(False, False), (False, True)] + ([(True, True)] if kind != "reach" else []) + ([(True, False)] if kind == "pick_place" else [])
        counts = {g: int(((mm == g[0]) & (et == g[1])).sum()) for g in groups}
        assert all(c >= MIN_PER_GROUP for c in counts.values()), f"{kind}: rows per (mismatch, verdict) {counts}"
        print(kind, "rows per (gripped mismatch, early termination):", counts)
    data.update(params=np.array(repr(PARAMS)),
                note=np.array("outputs of human_robot_gym's ReachHuman / PickPlaceHumanCart / CollaborativeLiftingCart StateBasedExpertImitationRewardWrapper "
                              "._get_imitation_reward and ._should_terminate_early (objects made with object.__new__ + their private parameters; pick-place: m_sim_fn = the "
                              "name in the key, g_sim_fn = the other one), run with stand-ins: bare package shells for human_robot_gym, .utils, .demonstrations, .wrappers; "
                              "gym = {Space, Env, Wrapper, core.Env, spaces.Box}; robosuite.environments.MujocoEnv, robosuite.wrappers.{Wrapper, GymWrapper} empty classes; "
                              "utils.mjcf_utils.file_path_completion = identity.  Inputs are rows of the 64-column observation superset (f32); rows within 1e-9 of an early "
                              "termination threshold dropped; r_motion / r_gripper are NaN where the wrapper appended none"))
    np.savez_compressed(out, **data)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
