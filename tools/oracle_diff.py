#!/usr/bin/env python3
"""Drive two builds of the CPU oracle side by side through a fixed corpus and compare every output and state byte.

    python tools/oracle_diff.py OLD.so NEW.so [SUBSTRING]      # only the runs whose label contains SUBSTRING

After reset and after every policy step obs, term_obs, reward, done, info, the (rewritten) action rows, contacts() and every state block of
get_states_all() are compared with == on raw bytes.  Prints the first differing case / step / env / field and exits 1; exits 0 when nothing differs.
The corpus: every case of make_golden.CASES x robot_geometry {capsule, hull} x {joint, IK} actions x done_at_success {True, False}, one run per
shield type of each stepper family, a cube carried between the fingers, and scripted events (deliveries, a reached joint goal, the hammer laid on
the nail, task phases forced to COMPLETE) that take every family through its _on_goal_reached branch.  80 policy steps of 8 envs each."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import human_robot_gym_amd as hrg  # noqa: E402
from human_robot_gym_amd._cstruct import CONST  # noqa: E402
from human_robot_gym_amd.mixed import task_env_kwargs  # noqa: E402
from oracle.oracle import OracleBatch  # noqa: E402
from tools.make_golden import CASES, clips_for  # noqa: E402
import pp_scenarios  # noqa: E402

N_ENVS, N_STEPS, SEED = 8, 80, 11
IK = dict(action_limit=0.15)
# the phase value `_check_success` waits for, per env_id: forced once per run (step 30) where done_at_success is False
COMPLETE = {"HumanObjectInspectionCart": "HRG_PHASE_COMPLETE", "HumanRobotHandoverCart": "HRG_PHASE_COMPLETE", "CollaborativeLiftingCart": "HRG_PHASE_COMPLETE",
            "RobotHumanHandoverCart": "HRG_R2H_COMPLETE", "CollaborativeStackingCart": "HRG_STK_COMPLETE", "CollaborativeHammeringCart": "HRG_HM_COMPLETE"}
FAMILIES = {"reach_ssm": "ReachHuman", "pick_place_ssm": "PickPlaceHumanCart", "stacking_ssm": "CollaborativeStackingCart", "hammering_ssm": "CollaborativeHammeringCart"}


def corpus():
    """(label, case name, env kwargs overrides, build_model_desc kwargs, scenario)"""
    for name in CASES:
        for geom in ("capsule", "hull"):
            for ik in (False, True):
                for das in (True, False):
                    yield (f"{name}/{geom}/{'ik' if ik else 'joint'}/das={int(das)}", name, dict(done_at_success=das),
                           dict(robot_geometry=geom, ik_position_delta=IK if ik else None), "golden")
    for name in FAMILIES:
        for shield in ("OFF", "SSM", "PFL"):
            yield f"{name}/shield={shield}", name, dict(shield_type=shield, done_at_success=False), {}, "golden"
    for geom in ("capsule", "hull"):
        yield f"pick_place_ssm/{geom}/grasp_and_carry", "pick_place_ssm", dict(horizon=100), dict(robot_geometry=geom), "carry"


def force_complete(batches, env_id):
    """The task phase of every env to its COMPLETE value, through the block setters."""
    kind = dict(box=env_id not in ("CollaborativeStackingCart", "CollaborativeHammeringCart"), stack=env_id == "CollaborativeStackingCart",
                hammer=env_id == "CollaborativeHammeringCart")
    for B in batches:
        st, bx, sk, hm = B.get_states_all(**kind)
        for blk in (bx, sk, hm):
            if blk is not None:
                for e in range(B.n):
                    blk[e].task_phase = CONST[COMPLETE[env_id]]
        B.set_states_all(None, bx, sk, hm)


def reach_goal(batches):
    """ReachHuman: the goal moved onto the arm's current configuration, so that this step reaches it (-> next goal)."""
    for B in batches:
        for e in range(B.n):
            st = B.get_state(e)
            st.cur_goal[:] = list(st.qpos)[:len(st.cur_goal)]
            B.set_state(e, st)


def hammer_on_nail(batches, desc):
    """The hammer laid on the nail head, handle level, at rest (as tests/test_hammering.py does): head - nail contacts, the nail's slide DoF in contact rows."""
    for B in batches:
        for e in range(B.n):
            hm = B.get_hammer(e)
            w, x, y, z = hm.quat[0]
            Rb = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                           [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
            top = np.array(hm.pos[0]) + Rb @ np.array([hm.nail_xy[0], hm.nail_xy[1], desc.hm_nail_z0 + 0.003])
            hm.quat[1][:] = [np.sqrt(0.5), 0, np.sqrt(0.5), 0]  # turned 90 deg about y: the head's x axis is vertical
            Rh = np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])
            head = np.array(desc.hm_geom_pos[CONST["HRG_HG_HEAD"]][:])
            hm.pos[1][:] = (top + [0, 0, desc.hm_geom_half[CONST["HRG_HG_HEAD"]][0]] - Rh @ head).tolist()
            hm.vel[1][:] = [0.0] * 6
            B.set_hammer(e, hm)


def arrays(B, stepped):
    """[(field name, array [n_envs, ...])] of what a reset / a step hands back"""
    pairs, ncon = B.contacts()
    names = ("obs", "term_obs", "reward", "done", "info", "last_actions") if stepped else ("obs",)
    return [(f, getattr(B, f)) for f in names] + [("contacts.pairs", pairs), ("contacts.ncon", ncon)]


def first_difference(A, B, stepped):
    """(env, field) of the first differing byte, or None"""
    for (f, a), (_, b) in zip(arrays(A, stepped), arrays(B, stepped)):
        if a.tobytes() != b.tobytes():
            return next(e for e in range(A.n) if a[e].tobytes() != b[e].tobytes()), f
    for sa, sb in zip(A.get_states_all(box=True, stack=True, hammer=True), B.get_states_all(box=True, stack=True, hammer=True)):
        if bytes(sa) == bytes(sb):
            continue
        T = type(sa[0])
        e = next(e for e in range(A.n) if bytes(sa[e]) != bytes(sb[e]))
        for fname, _ in T._fields_:
            off, size = getattr(T, fname).offset, getattr(T, fname).size
            if bytes(sa[e])[off:off + size] != bytes(sb[e])[off:off + size]:
                return e, f"{T.__name__}.{fname}"
        return e, f"{T.__name__} (padding)"
    return None


def run(label, name, kw_over, build_kw, scenario, libs):
    kw = dict(CASES[name])
    kw.update(kw_over)
    env_id = kw.pop("env_id", "ReachHuman")
    kw.update(task_env_kwargs(env_id))
    clips = clips_for(name)
    desc = hrg.build_model_desc(kw, n_clips=clips.n_clips, env_id=env_id, **build_kw)
    batches = [OracleBatch(desc, clips, N_ENVS, lib_path=p) for p in libs]
    for B in batches:
        B.reset()
    diff = first_difference(*batches, stepped=False)
    if diff:
        return ("reset",) + diff
    rng = np.random.RandomState(SEED)
    for k in range(N_STEPS):
        a = rng.uniform(-1, 1, (N_ENVS, 7))  # as make_golden.run draws them
        if env_id not in ("ReachHuman", "PickPlaceHumanCart"):
            a[:, :6] *= 0.2
        if name == "contact_static":
            a[:, 1] = np.where(np.arange(N_ENVS) % 2 == 0, 1.0, -1.0)
            a[:, [0, 2, 3, 4, 5]] *= 0.2
        if scenario == "carry":
            a = pp_scenarios.grasp_and_carry(k, batches, rng, N_ENVS, desc)
        elif env_id == "PickPlaceHumanCart" and k in (20, 50):  # a delivery: cube teleported next to its target
            for e in range(N_ENVS):
                bx = batches[0].get_box(e)
                pp_scenarios.put_box(batches, e, pos=[bx.target[0] + 0.02, bx.target[1], 0.845], zero_warm=False)
        if env_id == "CollaborativeHammeringCart" and k == 12:
            hammer_on_nail(batches, desc)
        if env_id == "ReachHuman" and k == 30:
            reach_goal(batches)
        if env_id in COMPLETE and not kw.get("done_at_success", True) and k == 30:
            force_complete(batches, env_id)
        for B in batches:
            B.step(a.copy())
        diff = first_difference(*batches, stepped=True)
        if diff:
            return (f"step {k}",) + diff
    for B in batches:
        B.close()
    return None


def main(argv):
    if len(argv) not in (3, 4):
        print(__doc__)
        return 2
    libs = [os.path.abspath(p) for p in argv[1:3]]
    n = 0
    for label, name, kw_over, build_kw, scenario in corpus():
        if len(argv) == 4 and argv[3] not in label:
            continue
        diff = run(label, name, kw_over, build_kw, scenario, libs)
        if diff:
            print(f"DIFFERENT: case {label}, {diff[0]}, env {diff[1]}, field {diff[2]}")
            return 1
        n += 1
    print(f"{n} runs x {N_STEPS} steps x {N_ENVS} envs: 0 differing bytes between {argv[1]} and {argv[2]}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
