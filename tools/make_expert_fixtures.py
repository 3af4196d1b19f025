#!/usr/bin/env python3
"""Record what the reference's scripted experts and similarity functions compute: python tools/make_expert_fixtures.py REFERENCE_CHECKOUT [OUT.npz]

Runs the reference's own classes (human_robot_gym/demonstrations/experts/, utils/expert_imitation_reward_utils.py) on recorded inputs and writes
tests/golden/expert_ref.npz: inputs, parameters, outputs.  Build machine only: no test reads the checkout.

Stand-ins (recorded in the file's `note`): the expert modules need numpy and `gym.spaces.Box` only, but `import human_robot_gym` runs the package
__init__, which imports robosuite.  So bare package shells are registered for `human_robot_gym`, `.utils` and `.demonstrations` (their __init__ files
are not executed; the modules below them load from the checkout unchanged), and a `gym` module that carries only `Space` and `spaces.Box(low, high)`.

Parameters are the expert nodes of training/config_icra_2024/environment_evaluation/training/{R,PP,CL}-AIR.yaml (and the hammering expert's
defaults: no run config ships for it), with signal_to_noise_ratio = 1: the noise draws of the reference (numpy's PCG64) are not reproduced by the
stepper's counter hash, and at 1 they cannot show.
"""
import os
import sys
import types

import numpy as np

ROWS = 321          # one full 256-thread block + 65
MARGIN = 1e-9       # rows with a predicate this close to its threshold are dropped
PER_BRANCH = 40     # rows asked of every motion branch of the pick-place expert (at least 20 must come out)
PP_PARAMS = dict(hover_dist=0.2, tan_theta=0.5, horizontal_epsilon=0.035, vertical_epsilon=0.015, goal_dist=0.08, gripper_fully_opened_threshold=0.02,
                 release_when_delivered=True, delta_time=0.01)                                   # PP-AIR.yaml expert
CL_PARAMS = dict(board_size=[1.0, 0.4, 0.03], human_grip_offset=0.1, delta_time=0.01)            # CL-AIR.yaml expert
CART_LOW, CART_HIGH = [-0.1, -0.1, -0.1, -1.0], [0.1, 0.1, 0.1, 1.0]                              # ik_position_delta.action_limit 0.1 + gripper
JOINT_LOW, JOINT_HIGH = [-1.0] * 7, [1.0] * 7


def install_stand_ins(ref):
    gym, spaces = types.ModuleType("gym"), types.ModuleType("gym.spaces")

    class Space:
        pass

    class Box(Space):
        def __init__(self, low, high, dtype=np.float64):
            self.low, self.high = np.asarray(low, dtype), np.asarray(high, dtype)
            self.shape = self.low.shape

    gym.Space, gym.spaces, spaces.Box = Space, spaces, Box
    sys.modules["gym"], sys.modules["gym.spaces"] = gym, spaces
    root = os.path.join(ref, "human_robot_gym")
    for name, sub in (("human_robot_gym", ""), ("human_robot_gym.utils", "utils"), ("human_robot_gym.demonstrations", "demonstrations")):
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(root, sub)]
        sys.modules[name] = m
    return Box


def f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def main():
    ref = os.path.abspath(sys.argv[1])
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(here, "tests", "golden", "expert_ref.npz")
    sys.path.insert(0, os.path.join(here, "tests"))
    import expert_ref as R   # margins of the predicates (which rows to drop); the recorded outputs below are the reference's alone
    Box = install_stand_ins(ref)
    from human_robot_gym.demonstrations.experts import (CollaborativeHammeringCartExpert, CollaborativeLiftingCartExpert, PickPlaceHumanCartExpert,
                                                        ReachHumanExpert)
    from human_robot_gym.utils.expert_imitation_reward_utils import similarity_fn
    rng = np.random.RandomState(20240)
    obs_space = Box([-np.inf] * 4, [np.inf] * 4)
    cart, joint = Box(CART_LOW, CART_HIGH), Box(JOINT_LOW, JOINT_HIGH)
    data = {}

    # ---- ReachHumanExpert: goal differences inside and beyond the action bounds
    ex = ReachHumanExpert(obs_space, joint, signal_to_noise_ratio=1, delta_time=0.01, seed=0)
    gd = f32(rng.uniform(-1.5, 1.5, (ROWS, 6)) * rng.choice([1.0, 0.1], (ROWS, 1)))
    data["reach_goal_difference"] = gd
    data["reach_action"] = np.array([ex(dict(goal_difference=g)) for g in gd])

    # ---- PickPlaceHumanCartExpert: a pool, labelled with the reference's own predicates, stratified over its 5 motion x 3 gripper branches
    ex = PickPlaceHumanCartExpert(obs_space, cart, signal_to_noise_ratio=1, seed=0, **PP_PARAMS)
    n_pool = 20000
    o2o = rng.uniform(-0.3, 0.3, (n_pool, 3)) * rng.choice([1.0, 0.1, 0.01], (n_pool, 1))
    o2t = rng.uniform(-0.3, 0.3, (n_pool, 3)) * rng.choice([1.0, 0.1], (n_pool, 1))
    near = rng.rand(n_pool) < 0.3
    o2t[near] = o2o[near] + rng.uniform(-0.05, 0.05, (int(near.sum()), 3))
    o2o, o2t = f32(o2o), f32(o2t)
    qpos = f32(np.stack([rng.uniform(0, 0.021, n_pool), -rng.uniform(0, 0.021, n_pool)], axis=1))
    gripped = rng.rand(n_pool) < 0.4
    _, margin = R.pick_place_predicates(gripped, o2o, o2t, qpos, **PP_PARAMS)
    keep = margin >= MARGIN
    dropped = 1.0 - keep.mean()
    assert dropped <= 0.01, f"{dropped:.4f} of the pool lies within {MARGIN} of a threshold"
    mb, gb = np.empty(n_pool, np.int64), np.empty(n_pool, np.int64)
    for i in range(n_pool):
        ob = ex.expert_observation_from_dict(dict(object_gripped=bool(gripped[i]), vec_eef_to_object=o2o[i], vec_eef_to_target=o2t[i], robot0_gripper_qpos=qpos[i]))
        dl, op = ex._object_delivered(ob), ex._gripper_fully_opened(ob)
        mb[i] = 0 if dl and op else 1 if ex._above_object(ob) and op else 2 if ex._above_target(ob) and ob.object_gripped else 3 if ob.object_gripped else 4
        gb[i] = 0 if dl and ex._release_when_delivered else 1 if ob.object_gripped or ex._at_object(ob) else 2
    chosen = []
    for b in range(5):
        idx = np.nonzero(keep & (mb == b))[0]
        chosen += idx[:PER_BRANCH].tolist()
    for b in range(3):
        idx = [i for i in np.nonzero(keep & (gb == b))[0].tolist() if i not in chosen]
        chosen += idx[:PER_BRANCH]
    rest = [i for i in np.nonzero(keep)[0].tolist() if i not in set(chosen)]
    chosen = np.array((chosen + rest)[:ROWS])
    chosen = chosen[rng.permutation(ROWS)]
    assert len(chosen) == ROWS and all((mb[chosen] == b).sum() >= 20 for b in range(5)) and all((gb[chosen] == b).sum() >= 20 for b in range(3))
    data.update(pp_object_gripped=gripped[chosen], pp_vec_eef_to_object=o2o[chosen], pp_vec_eef_to_target=o2t[chosen], pp_robot0_gripper_qpos=qpos[chosen],
                pp_motion_branch=mb[chosen], pp_gripper_branch=gb[chosen], pp_dropped_share=np.float64(dropped))
    data["pp_action"] = np.array([ex(dict(object_gripped=bool(gripped[i]), vec_eef_to_object=o2o[i], vec_eef_to_target=o2t[i], robot0_gripper_qpos=qpos[i])) for i in chosen])

    # ---- CollaborativeLiftingCartExpert: hands 0.3 - 1.3 m in front of the gripper, half a metre apart
    ex = CollaborativeLiftingCartExpert(obs_space, cart, signal_to_noise_ratio=1, seed=0, **CL_PARAMS)
    mid = rng.uniform([0.3, -0.4, -0.3], [1.3, 0.4, 0.3], (ROWS, 3)) * rng.choice([1.0, 0.2], (ROWS, 1))
    half = rng.uniform(-0.05, 0.05, (ROWS, 3)) + np.array([0.0, 0.25, 0.0])
    lh, rh = f32(mid + half), f32(mid - half)
    data.update(cl_vec_eef_to_human_lh=lh, cl_vec_eef_to_human_rh=rh)
    data["cl_action"] = np.array([ex(dict(vec_eef_to_human_lh=a, vec_eef_to_human_rh=b, board_quat=np.array([0.0, 0.0, 0.0, 1.0]), board_gripped=True)) for a, b in zip(lh, rh)])

    # ---- CollaborativeHammeringCartExpert
    ex = CollaborativeHammeringCartExpert(obs_space, cart, signal_to_noise_ratio=1, seed=0)
    nail = f32(rng.uniform(-0.4, 0.4, (ROWS, 3)) * rng.choice([1.0, 0.2], (ROWS, 1)))
    data["hm_vec_eef_to_nail"] = nail
    data["hm_action"] = np.array([ex(dict(vec_eef_to_nail=v)) for v in nail])

    # ---- similarity_fn on a grid of distances x scales
    delta = np.concatenate([[0.0], np.logspace(-6, 1, 57)])
    iota = np.array([0.05, 0.1, 0.25, 0.5])
    data.update(sim_delta=delta, sim_iota=iota)
    for name in ("gaussian", "tanh"):
        data["sim_" + name] = np.array([[similarity_fn(name, d, i) for i in iota] for d in delta])

    data.update(cart_low=np.array(CART_LOW), cart_high=np.array(CART_HIGH), joint_low=np.array(JOINT_LOW), joint_high=np.array(JOINT_HIGH),
                pp_params=np.array(repr(PP_PARAMS)), cl_params=np.array(repr(CL_PARAMS)),
                note=np.array("outputs of human_robot_gym's ReachHumanExpert, PickPlaceHumanCartExpert, CollaborativeLiftingCartExpert, CollaborativeHammeringCartExpert "
                              "(signal_to_noise_ratio=1) and similarity_fn, run with stand-ins: bare package shells for human_robot_gym, .utils, .demonstrations "
                              "(their __init__ not executed), gym = {Space, spaces.Box(low, high)}; inputs f32-representable; pick-place rows within 1e-9 of a "
                              "predicate threshold dropped"))
    np.savez_compressed(out, **data)
    print("wrote", out, os.path.getsize(out), "bytes; pick-place dropped share", dropped, "motion branches", np.bincount(mb[chosen], minlength=5),
          "gripper branches", np.bincount(gb[chosen], minlength=3))


if __name__ == "__main__":
    main()
