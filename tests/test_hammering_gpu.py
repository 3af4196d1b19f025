"""CollaborativeHammeringCart: HIP stepper (hrg_step_kernel_hammer) vs CPU oracle on identical seeded inputs, through the C ABI.  -m gpu."""
import numpy as np
import pytest

import human_robot_gym_amd as hrg
from human_robot_gym_amd._cstruct import CONST
from human_robot_gym_amd.mixed import task_clips, task_env_kwargs
from helpers import make_pair, quat_mat
from parity import GEOM_BOX as G0, Run, pose_vectors

pytestmark = pytest.mark.gpu
ENV = "CollaborativeHammeringCart"


def _pair(n, kw, clips=None):
    O, G = make_pair(n, kw, clips=clips, task_frames=(300, 420), env_id=ENV)
    return O, G, O.desc


def _rollout(O, G, n, n_steps, seed, resync, name, scenario=None, min_live=0.9, act_scale=1.0, twin=None):
    """violent here: a violent arm, a crash, a free body that moves at > 3 m/s.  An env-step whose contact list differs at agreeing floats leaves the comparison
    (parity.Step.drop_flicker: free-running for good, resynchronised for this step), counted in `flicker` and bounded.
    `twin` (resynchronised runs): a second oracle batch that takes every step from the first one's state with the hammer moved by 1e-12 m.  An env whose two oracle
    results then differ by more than 1e-7 sits on a knife edge of the step itself (a box-box reference face or a noslip bound that flips within the 25 substeps: the
    fuzz scenario throws the hammer into the board at random poses) -- no implementation can be expected to land on the oracle's side of it.  Such env-steps leave the
    comparison, counted in `knife` and bounded."""
    run = Run(O, G, f"test_hammering_gpu::{name}", free_running=not resync)
    if twin is not None:
        twin.reset()
    rng = np.random.RandomState(seed)
    stats = dict(hammer_contacts=0, box_box=0, nail_contacts=0, phases=set(), max_ncon=0, gripped=0, static=0, flicker=0, knife=0)

    def actions(k):
        if scenario is not None:
            scenario(k, [O, G])
        a = rng.uniform(-1, 1, (n, 7)) * act_scale
        if twin is not None:
            for e in range(n):
                hm = O.get_hammer(e)
                hm.pos[1][0] += 1e-12
                twin.set_state(e, O.get_state(e)); twin.set_hammer(e, hm)
            twin.step(a.copy())
        return a
    for s in run.steps(n_steps, actions):
        if twin is not None:
            knife = np.abs(pose_vectors("hammer", s.o.objects) - pose_vectors("hammer", twin.get_states_all(hammer=True)[3])).max(axis=1) > 1e-7
            stats["knife"] += int((s.chk & knife).sum())
            s.chk &= ~knife
        s.drop_flicker()
        s.compare()
        po, chk = s.o.pairs, s.chk
        stats["hammer_contacts"] += int(((po[chk][:, :, 1] == G0 + 1) | (po[chk][:, :, 1] == G0 + 2)).sum())
        stats["box_box"] += int(((po[chk][:, :, 0] >= G0) & (po[chk][:, :, 1] >= G0)).sum())
        stats["nail_contacts"] += int((po[chk][:, :, 1] == G0 + 3).sum())
        stats["max_ncon"] = max(stats["max_ncon"], int(s.o.ncon[chk].max()) if chk.any() else 0)
        stats["static"] = max(stats["static"], int(s.o.info[chk, 3].max()) if chk.any() else 0)
        stats["phases"] |= {int(hm.task_phase) for hm in s.o.objects}
        stats["gripped"] += sum(int(hm.gripped) for hm in s.o.objects)
        if resync:
            s.resync()
    stats["flicker"] = run.flicker
    run.finish(min_live)
    assert stats["flicker"] <= max(2, (n * n_steps) // 100), f"{name}: {stats['flicker']} env-steps with a contact list that differs at agreeing bodies"
    assert stats["knife"] <= max(2, (n * n_steps) // 50), f"{name}: {stats['knife']} env-steps on a knife edge of the oracle itself"
    if twin is not None:
        print(f"[parity] {name}: {stats['knife']} of {n * n_steps} env-steps on a knife edge of the oracle (left out), {stats['flicker']} contact-list flickers")
        twin.close()
    return stats


@pytest.mark.parametrize("shield", ["OFF", "SSM"])
def test_random_actions_parity_resync(shield):
    """Per-step parity with the GPU state re-synchronised after every step: the board carried in by the human (weld + connect), the hammer pinched by the
    fingers, its grip contacts and the nail's friction row through the noslip pass, APPROACH -> PRESENT."""
    O, G, _ = _pair(12, dict(shield_type=shield, horizon=60, seed=2))
    st = _rollout(O, G, 12, 40, 1, True, f"random_{shield}", act_scale=0.3)
    assert st["hammer_contacts"] > 0 and st["gripped"] > 0 and {0, 1} <= st["phases"]


def test_random_actions_parity_free_running():
    O, G, _ = _pair(16, dict(shield_type="SSM", horizon=30, seed=3))
    st = _rollout(O, G, 16, 45, 2, False, "random_free", min_live=0.9, act_scale=0.3)   # incl. auto-resets (measured: 16 of 16 stay in)
    assert st["hammer_contacts"] > 0


def _on_the_nail(k, Bs):
    """Step 12: the hammer is laid onto the nail (env 0, 1: head on the nail head, handle level; env 2: dropped from 3 cm; env 3: head flat on the board)."""
    if k != 12:
        return
    for B in Bs:
        for e in range(4):
            hm = B.get_hammer(e)
            d = B.desc if hasattr(B, "desc") else None
            Rb = quat_mat(hm.quat[0])
            hm.nail_q = hm.nail_v = 0.0
            hm.quat[1][:] = [np.sqrt(0.5), 0, np.sqrt(0.5), 0]
            Rh = quat_mat(hm.quat[1])
            head = np.array([0.0, 0.0, 0.0875 + 0.01925 - 0.06726677713338856])
            if e < 3:
                top = np.array(hm.pos[0]) + Rb @ np.array([hm.nail_xy[0], hm.nail_xy[1], 0.086 + 0.003])
                lift = 0.0616 + (0.03 if e == 2 else -2e-4) + (0.01 if e == 1 else 0.0) * 0
            else:
                top = np.array(hm.pos[0]) + Rb @ np.array([hm.nail_xy[0] - 0.2, hm.nail_xy[1], 0.015])
                lift = 0.0616 - 2e-4
            hm.pos[1][:] = (top + [0, 0, lift] - Rh @ head).tolist()
            hm.vel[1][:] = [0.0] * 6
            hm.acc_warmstart[1][:] = [0.0] * 6
            B.set_hammer(e, hm)


def _nail_at_the_finger(k, Bs):
    """Step 3: env 0's board is moved so that the nail head sits at a finger bar (robot - nail contacts: a static collision, rows on the board and the slide joint)."""
    if k != 3:
        return
    for B in Bs:
        hm, st = B.get_hammer(0), B.get_state(0)
        Rb = quat_mat(hm.quat[0])
        nail = Rb @ np.array([hm.nail_xy[0], hm.nail_xy[1], 0.086])
        hm.pos[0][:] = (np.array(st.eef_pos) + [0.0, 0.03, -0.02] - nail).tolist()
        hm.pos[1][:] = [0.3, -0.8, 3.0]
        hm.vel[1][:] = [0.0] * 6
        B.set_hammer(0, hm)


def test_robot_nail_contact_parity():
    O, G, d = _pair(2, dict(shield_type="OFF", horizon=100, seed=7))
    st = _rollout(O, G, 2, 10, 4, True, "nail_finger", scenario=_nail_at_the_finger, act_scale=0.0)
    assert st["static"] >= 1   # (the weld pulls the board back within the step: the contact shows in the collision counters, not in the last substep's list)


def test_hammer_on_nail_and_board_parity():
    """Box-box contacts of boxes with different extents (head - nail, head / handle - board) through the coupled 24-DoF Newton step, the nail's slide joint under load."""
    O, G, d = _pair(4, dict(shield_type="OFF", horizon=100, seed=4))
    st = _rollout(O, G, 4, 22, 3, True, "on_nail", scenario=_on_the_nail, act_scale=0.0)
    assert st["box_box"] > 0 and st["nail_contacts"] > 0
    O, G, d = _pair(4, dict(shield_type="OFF", horizon=100, seed=4))
    _rollout(O, G, 4, 20, 3, False, "on_nail_free", scenario=_on_the_nail, act_scale=0.0, min_live=0.75)


def _strikes(k, Bs):
    """Step 12: the hammer is laid onto the nail head (env 0), dropped onto it at 1.5 m/s (env 1) and at 3 m/s (env 2), laid onto the board (env 3)."""
    if k != 12:
        return
    _on_the_nail(k, Bs)
    for B in Bs:
        for e, v in ((1, 1.5), (2, 3.0)):
            hm = B.get_hammer(e)
            hm.pos[1][2] += 0.01
            hm.vel[1][2] = -v
            B.set_hammer(e, hm)


@pytest.mark.parametrize("floss", [5.0, 0.5])
def test_noslip_pass_with_a_yielding_nail_parity(floss):
    """MuJoCo's noslip post-pass (1161) with the friction bound in play: a nail with a friction loss of 5 N / 0.5 N under a resting hammer (1 N) and under blows --
    holding, yielding, driven to its range limit -- step by step against the oracle, then free-running."""
    O, G, d = _pair(4, dict(shield_type="OFF", horizon=100, seed=4, nail_frictionloss=floss))
    st = _rollout(O, G, 4, 24, 3, True, f"noslip_{floss}", scenario=_strikes, act_scale=0.0)
    assert st["nail_contacts"] > 0
    O, G, d = _pair(4, dict(shield_type="OFF", horizon=100, seed=4, nail_frictionloss=floss))
    _rollout(O, G, 4, 20, 3, False, f"noslip_{floss}_free", scenario=_strikes, act_scale=0.0, min_live=0.75)


def test_scripted_episode_through_success_parity():
    """The whole phase machine on both steppers: the nail is pushed in by hand once the board is presented; RETREAT, COMPLETE, _on_goal_reached, next animation."""
    clips = task_clips(ENV, 2, min_frames=300, max_frames=340)
    O, G, d = _pair(2, dict(shield_type="OFF", horizon=400, seed=5, done_at_success=False, nail_hammered_in_reward=-0.5, hammer_gripped_reward_bonus=0.25), clips=clips)
    done_once = {}

    def scenario(k, Bs):
        for e in range(2):
            hm = Bs[0].get_hammer(e)
            if hm.task_phase == CONST["HRG_HM_PRESENT"] and k >= 24 and not done_once.get((e, hm.nail_index)):
                for B in Bs:
                    h2 = B.get_hammer(e)
                    h2.nail_q, h2.nail_v = d.hm_nail_range, 0.0
                    B.set_hammer(e, h2)
                done_once[(e, hm.nail_index)] = True
    st = _rollout(O, G, 2, 110, 6, True, "scripted", scenario=scenario, act_scale=0.0)
    assert st["phases"] >= {0, 1, 3}


def test_box_box_fuzz_parity():
    """Box-box contacts of boxes with different extents, fuzzed: every other step the hammer of every env is thrown at the board / the nail in a random pose
    (head or handle a few millimetres inside the board's top face, tilted up to 35 deg, or the head on the nail), then one step on both steppers from
    the same state.  Face / edge / vertex configurations of the SAT + clipping code with unequal half extents, the coupled 24-DoF Newton step, the nail's rows."""
    n = 48
    O, G, d = _pair(n, dict(shield_type="OFF", horizon=200, seed=9))
    rs = np.random.RandomState(5)

    def scenario(k, Bs):
        if k < 3 or k % 2 == 0:
            return
        hm0 = [Bs[0].get_hammer(e) for e in range(n)]
        poses = []
        for e in range(n):
            hm = hm0[e]
            Rb = quat_mat(hm.quat[0])
            ax = rs.randn(3); ax /= np.linalg.norm(ax)
            ang = rs.uniform(0, 0.6)
            qt = np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * ax])
            base = np.array([np.sqrt(0.5), 0, np.sqrt(0.5), 0])                    # handle level, head pointing down
            w1, v1, w2, v2 = qt[0], qt[1:], base[0], base[1:]
            q = np.concatenate([[w1 * w2 - v1 @ v2], w1 * v2 + w2 * v1 + np.cross(v1, v2)])
            Rh = quat_mat(q)
            head = np.array([0.0, 0.0, 0.0875 + 0.01925 - 0.06726677713338856])
            if e % 3 == 0:    # head over the nail
                tgt = np.array(hm.pos[0]) + Rb @ np.array([hm.nail_xy[0], hm.nail_xy[1], 0.086 + 0.003 + 0.0616 - rs.uniform(0, 0.004)])
            else:             # head over a random spot of the board's nail half
                tgt = np.array(hm.pos[0]) + Rb @ np.array([rs.uniform(-0.3, 0.4), rs.uniform(-0.15, 0.15), 0.015 + 0.0616 - rs.uniform(0, 0.004)])
            poses.append((tgt - Rh @ head, q))
        for B in Bs:
            for e in range(n):
                hm = B.get_hammer(e)
                hm.pos[1][:] = poses[e][0].tolist(); hm.quat[1][:] = poses[e][1].tolist()
                hm.vel[1][:] = [0.0] * 6; hm.acc_warmstart[1][:] = [0.0] * 6
                B.set_hammer(e, hm)
    from oracle.oracle import OracleBatch
    clips = task_clips(ENV, 3, min_frames=300, max_frames=420)
    O2 = OracleBatch(hrg.build_model_desc(dict(task_env_kwargs(ENV), shield_type="OFF", horizon=200, seed=9), n_clips=clips.n_clips, env_id=ENV), clips, n)
    st = _rollout(O, G, n, 16, 8, True, "boxbox_fuzz", scenario=scenario, act_scale=0.0, twin=O2)
    assert st["box_box"] > 20 * 4
