"""CollaborativeLiftingCart (collaborative_lifting_cartesian_env.py): robot and human carry a board; the human's end hangs on two connect
equalities at the hand mocap bodies, the robot's end sits between the fingers.  PARITY UNPINNED: behaviour the reference
documents (rewards, termination rules, success = animation complete) on the CPU oracle, oracle <-> HIP parity on the GPU."""
import math

import numpy as np
import pytest

import human_robot_gym_amd as hrg
from human_robot_gym_amd import mixed
from human_robot_gym_amd._cstruct import CONST
from human_robot_gym_amd.animation import hand_sites, lifting_hands_nominal

ENV = "CollaborativeLiftingCart"


def _clips(n=3, lo=100, hi=150):
    return mixed.task_clips(ENV, n, min_frames=lo, max_frames=hi)


def _oracle(n, kw, clips):
    from oracle.oracle import OracleBatch
    d = hrg.build_model_desc(kw, n_clips=clips.n_clips, env_id=ENV)
    return OracleBatch(d, clips, n), d


def test_desc_follows_the_reference_defaults():
    d = hrg.build_model_desc(None, env_id=ENV)
    assert d.task == CONST["HRG_TASK_LIFTING"] and d.horizon == 5000 and d.n_anim_ids == 10      # collaborative_lifting_cart.yaml
    assert list(d.box_half) == [0.5, 0.2, 0.015] and abs(d.box_mass - 20 * 1.0 * 0.4 * 0.03) < 1e-12   # board_full_size, density 20 (755-760)
    assert d.min_balance == 0.8 and d.imbalance_failure_reward == -10 and d.board_released_reward == -10 and d.reward_shaping == 1
    assert [list(a) for a in d.lift_anchor] == [[-0.45, 0.25, 0.0], [-0.45, -0.25, 0.0]]          # _postprocess_model, 786-795
    assert np.allclose(list(d.init_qpos), [0, math.pi * 19 / 48, -math.pi / 2 - 5 * math.pi / 48, 0, math.pi / 2, -math.pi / 4], atol=1e-15)   # _reset_internal, 673


def test_synthetic_lifting_clips_put_the_hands_at_the_board_grips():
    d = hrg.build_model_desc(None, env_id=ENV)
    nom = lifting_hands_nominal(d)
    clips = _clips()
    o = 0
    for c in range(clips.n_clips):
        lh, rh = hand_sites(clips.frames[o:o + clips.lengths[c]], clips.infos[c])
        o += clips.lengths[c]
        mid = 0.5 * (lh + rh)
        assert np.allclose(mid[0], nom, atol=1e-9) and np.allclose(mid[-1], nom, atol=0.05)       # starts and ends at the board's rest height
        assert 0.55 < mid[:, 2].max() - nom[2] < 0.71                                             # the lift in between
        assert (lh[:, 1] < rh[:, 1]).all()                                                        # facing the robot: left hand at -y
        assert 0.3 < np.linalg.norm(rh - lh, axis=1).min() and np.linalg.norm(rh - lh, axis=1).max() < 0.7


def test_reset_puts_the_board_into_the_gripper_and_the_hands():
    B, d = _oracle(3, dict(seed=3, horizon=200), _clips())
    obs = B.reset()
    for e in range(3):
        bx, st = B.get_box(e), B.get_state(e)
        assert bx.weld_active == 1 and bx.task_phase == 0 and bx.n_delayed == 0
        assert obs[e, 50] > 0.995 and obs[e, 39] == 0                       # level (init noise 0.02 rad), not gripped yet: the fingers start open
        eef, pos = np.array(list(st.eef_pos)), np.array(list(bx.pos))
        assert abs(np.linalg.norm(pos - eef) - d.box_half[0]) < 1e-9        # robot-side edge at the grip site
        assert np.linalg.norm(np.array(list(bx.mocap_pos)) - np.array(list(bx.weld_off))) > 0.3   # the two hand mocap bodies
        assert np.allclose(obs[e, 47:50], pos, atol=1e-6) and np.allclose(obs[e, 40:43], pos - eef, atol=1e-6)
    B.close()


def test_holding_the_board_pays_the_balance_reward_and_losing_it_ends_the_episode():
    B, d = _oracle(4, dict(seed=3, horizon=200), _clips())
    B.reset()
    held = 0
    ended = {"imbalance": 0, "released": 0}
    unheld = np.zeros(4, int)
    for k in range(60):
        obs, r, dn, info = B.step(np.zeros((4, 7)))                          # the gripper action is overridden by 'close' (368-391)
        t = B.term_obs
        for e in range(4):
            bal, grip = float(t[e, 50]), t[e, 39] != 0
            unheld[e] = 0 if grip else unheld[e] + 1
            dense = (math.asin(min(bal, 1.0)) * 2 / math.pi - math.asin(0.8) * 2 / math.pi) / (1 - math.asin(0.8) * 2 / math.pi) - 2.0
            sparse = -10.0 if bal < 0.8 else (-10.0 if not grip else 1.0)   # _sparse_reward, 446-478 (no success in this window)
            assert abs(r[e] - (sparse + 1.0 + dense)) < 2e-5, (k, e, r[e], bal, grip)
            assert bool(dn[e]) == (bal < 0.8 or unheld[e] > 5)               # _check_done, 509-561
            if dn[e]:
                ended["imbalance" if bal < 0.8 else "released"] += 1
                unheld[e] = 0
            held += int(grip and bal >= 0.8)
        assert not info[:, 11].any()
    assert held > 60 and ended["imbalance"] + ended["released"] > 0          # the robot stands still while the human lifts: the board slips out sooner or later
    B.close()


def test_a_released_board_comes_to_rest_on_the_table():
    """The table of the lifting task (TableArena: 0.4 x 1.5 m, its top 0.8 m high, one metre in front of the robot: collaborative_lifting_cartesian_env.py:280-284,
    742-746) lies under the board's middle.  Let go by the human (connects off) and by the robot (gripper opened), the board -- 9 cm above it at the reset --
    drops onto the slab and stays there: box-box contacts between board and table (they overlap in a cross: no corner of one lies over the other), not the floor."""
    B, d = _oracle(1, dict(seed=3, horizon=400, done_at_collision=False), _clips())
    B.reset()
    assert list(d.table_center) == [1.0, 0.0] and list(d.table_half) == [0.2, 0.75] and d.table_top_z == 0.8
    assert B.get_box(0).pos[2] - d.box_half[2] > d.table_top_z + 0.05
    bx = B.get_box(0)
    bx.weld_active = 0
    B.set_box(0, bx)
    G_TABLE, G_BOX = 10 + 24, 10 + 24 + 2
    zs, on_table = [], 0
    for k in range(40):
        a = np.zeros((1, 7)); a[0, 6] = -1.0                           # open the gripper
        o, r, dn, i = B.step(a)
        if dn[0]:
            break                                                      # (the episode ends a few steps after the grip is lost: _check_done, 509-561)
        pairs, n = B.contacts()
        on_table += int(any(tuple(p) == (G_TABLE, G_BOX) for p in pairs[0][:n[0]].tolist()))
        zs.append(B.get_box(0).pos[2])
    assert k >= 5 and on_table >= 3
    assert d.table_top_z + d.box_half[2] - 0.005 < zs[-1] < d.table_top_z + d.box_half[2] + 0.03      # on the slab (its robot-side end still leans on a finger), not on the floor
    assert abs(zs[-1] - zs[-2]) < 2e-3
    B.close()


def test_animation_complete_is_the_success_and_starts_the_next_task():
    nominal = lifting_hands_nominal(hrg.build_model_desc(None, env_id=ENV))
    clips = hrg.synthetic_clips(2, fps=20.0, lifting=nominal, lift_height=0.1, min_frames=20, max_frames=24)   # 1.0-1.2 s, a 10 cm lift: over after 10-12 policy steps
    B, d = _oracle(2, dict(seed=5, horizon=200, done_at_success=False), clips)
    B.reset()
    wins, checked = np.zeros(2, int), 0
    for k in range(40):
        obs, r, dn, info = B.step(np.zeros((2, 7)))
        for e in range(2):
            if info[e, 9] > wins[e]:                                           # n_goal_reached went up: task_reward (+ shaping), robot and board back at the start
                wins[e] = info[e, 9]
                assert r[e] > -1.0                                  # task_reward + 1 + (normalised balance - 2); a failure would pay -10
                if dn[e]:                                           # (the board may have slipped in the same step: _check_done is independent)
                    continue
                checked += 1
                bx, st = B.get_box(e), B.get_state(e)
                assert bx.task_phase == 0 and np.allclose(list(st.qpos)[:6], list(d.init_qpos), atol=1e-12) and max(abs(v) for v in st.qvel) == 0
                assert abs(np.linalg.norm(np.array(list(bx.pos)) - np.array(list(st.eef_pos))) - d.box_half[0]) < 1e-9
    assert (wins >= 1).all() and checked >= 1
    B2, _ = _oracle(2, dict(seed=5, horizon=200, done_at_success=True), clips)
    B2.reset()
    done_on_success = 0
    for k in range(30):
        obs, r, dn, info = B2.step(np.zeros((2, 7)))
        done_on_success += int(((info[:, 9] > 0) & (dn != 0)).sum())
    assert done_on_success >= 1
    B.close(); B2.close()


@pytest.mark.gpu
def test_hip_matches_oracle_on_the_lifting_task():
    from helpers import make_pair
    from parity import Run
    O, G = make_pair(6, dict(seed=3, horizon=40, shield_type="SSM"), clips=_clips(3, 100, 150), env_id=ENV)
    run = Run(O, G, "lifting", free_running=True, violent=None, atol=2e-6, reward_atol=2e-6)
    rng = np.random.RandomState(0)
    held = 0
    for s in run.steps(90, lambda k: rng.uniform(-0.3, 0.3, (6, 7))):
        s.compare()
        held += int(s.o.term_obs[:, 39].sum())
        if s.k % 4 == 3:      # three-point support with sliding finger contacts: resynchronise before rounding differences grow
            s.resync()
    assert held > 100
    run.finish()


@pytest.mark.gpu
def test_lifting_long_run_stays_finite():
    """Soak: 1024 envs x 200 policy steps of random arm actions with auto-resets: nothing turns non-finite, no simulation crashes, the board
    stays a rigid body, boards are held for a good part of the time and episodes end for every documented reason."""
    import torch
    from human_robot_gym_amd._lib import HipBatch
    n = 1024
    clips = _clips(5, 200, 400)
    d = hrg.build_model_desc(dict(seed=31, horizon=150), n_clips=clips.n_clips, env_id=ENV)
    G = HipBatch(d, clips, n)
    G.reset()
    g = torch.Generator(device="cpu").manual_seed(4)
    crashes = held = dones = 0
    for k in range(200):
        a = ((torch.rand((n, 7), generator=g, dtype=torch.float64) * 2 - 1) * 0.3).cuda()
        obs, r, dn, info = G.step(a)
        crashes += int(info[:, 11].sum().item()); dones += int(dn.sum().item())
        if k % 40 == 39:
            o, t = obs.cpu().numpy(), G.term_obs.cpu().numpy()
            assert np.isfinite(o).all() and np.isfinite(t).all() and np.isfinite(r.cpu().numpy()).all()
            held += int((t[:, 39] != 0).sum())
            _, bx = G.get_states(np.arange(0, n, 16))
            assert max(abs(np.linalg.norm(list(b.quat)) - 1) for b in bx) < 1e-12
            assert all(b.weld_active == 1 for b in bx)
    assert crashes == 0 and held > n and dones > 0
    G.close()


def test_board_on_its_two_connects_swings_like_a_physical_pendulum():
    """Known answer for the connect rows (point Jacobian [1 | -[r]x]) and the anisotropic inertia: with the robot out of the way the board
    hangs on the line through its two anchors; small swings have the period 2 pi sqrt((I_yy + m d^2) / (m g d)), d = 0.45 m."""
    from human_robot_gym_amd.animation import ClipSet, _qpos_joint_order
    from oracle.oracle import OracleBatch
    src = _clips(1, 100, 120)
    f0, order = src.frames[0], _qpos_joint_order()
    n = 900
    anim = {"Pelvis_pos_x": np.full(n, f0[0]), "Pelvis_pos_y": np.full(n, f0[1]), "Pelvis_pos_z": np.full(n, f0[2]), "Pelvis_quat": np.tile(f0[3:7], (n, 1))}
    anim.update({name: np.full(n, f0[7 + k]) for k, name in enumerate(order)})
    clips = ClipSet([(anim, src.infos[0])])                       # the human stands still: the hands (mocap bodies) are fixed points
    d = hrg.build_model_desc(dict(seed=1, horizon=2000, control_freq=50, shield_type="OFF", min_balance=-0.99, done_at_success=False,
                                  base_human_pos_offset=[0.0, 0.0, 0.6]), n_clips=1, env_id=ENV)      # the human on a 60 cm step: the 1 m board clears the floor
    B = OracleBatch(d, clips, 1)
    B.reset()
    st, bx = B.get_state(0), B.get_box(0)
    for j, q in enumerate([0.0, -1.2, 0.0, 0.0, 0.0, 0.0]):      # the arm folded back over the base, away from the board
        st.qpos[j] = q
    for k in range(len(st.ltt.q0)):
        st.ltt.q0[k] = st.ltt.qT[k] = st.des_q[k] = st.goal_qpos[k] = st.new_goal_q[k] = st.qpos[k]
    B.set_state(0, st)
    hl, hr = np.array(list(bx.mocap_pos)), np.array(list(bx.weld_off))
    c, u = 0.5 * (hl + hr), (hr - hl) / np.linalg.norm(hr - hl)

    def rot(axis, ang):
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)

    def quat_of(R):
        w = 0.5 * np.sqrt(max(1 + R[0, 0] + R[1, 1] + R[2, 2], 1e-30))
        return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])

    down = np.array([0.0, 0.0, -1.0]) - u * (np.array([0.0, 0.0, -1.0]) @ u)
    down /= np.linalg.norm(down)
    xb = rot(u, np.radians(10.0)) @ down                          # from the hinge line to the far edge: 10 degrees off the vertical
    yb = -u                                                       # the left anchor (+y in the board frame) at the left hand
    Rb = np.stack([xb, yb, np.cross(xb, yb)], 1)
    best = (c + 0.45 * xb, quat_of(Rb))                           # the anchors' midpoint (-0.45, 0, 0) on the hands' midpoint
    bx.pos[:] = best[0].tolist(); bx.quat[:] = best[1].tolist()
    for a in range(6):
        bx.vel[a] = 0.0; bx.acc_warmstart[a] = 0.0
    B.set_box(0, bx)
    phi = []
    for k in range(200):                                          # 4 s
        _, _, dn, info = B.step(np.zeros((1, 7)))
        assert not info[0, 11] and not dn[0]
        bx = B.get_box(0)
        bx.n_delayed = 0                                          # (nobody grips the board here: keep _check_done's 5-step tolerance from ending the episode)
        B.set_box(0, bx)
        r = np.array(list(bx.pos)) - c
        r -= u * (r @ u)
        phi.append(np.arctan2(np.cross(np.array([0, 0, -1.0]), r) @ u, -r[2]))
    phi = np.array(phi)
    up = [k for k in range(1, len(phi)) if phi[k - 1] < 0 <= phi[k]]
    assert len(up) >= 2 and 0.1 < np.abs(phi).max() < 0.25
    t_cross = [(k - 1 + (0 - phi[k - 1]) / (phi[k] - phi[k - 1])) * 0.02 for k in up]
    period = np.mean(np.diff(t_cross))
    m, dcom = d.box_mass, 0.45
    expect = 2 * np.pi * np.sqrt((d.box_inertia[1] + m * dcom ** 2) / (m * 9.81 * dcom))
    assert abs(period - expect) < 0.03 * expect, (period, expect)
    B.close()


def test_a_following_robot_carries_the_board_through_and_a_resting_one_tips_it():
    """The task as the reference poses it: the human raises their end by 60-70 cm and lowers it again.  Cartesian actions (IK front-end) that keep
    the gripper level with the middle of the hands bring every episode to its success; with zero actions the board tilts past min_balance."""
    from oracle.oracle import OracleBatch
    clips = mixed.task_clips(ENV, 2, min_frames=200, max_frames=240)        # 10-12 s at 20 Hz
    d = hrg.build_model_desc(dict(seed=2, horizon=400), n_clips=clips.n_clips, env_id=ENV, ik_position_delta=dict(action_limit=0.15))
    outcome = {}
    for follow in (True, False):
        B = OracleBatch(d, clips, 6)
        obs = B.reset()
        wins = fails = held = 0
        for k in range(135):
            mid = 0.5 * (obs[:, 0:3] + obs[:, 4:7])                             # eef -> middle of the hands (vec_eef_to_human_lh / rh)
            a = np.zeros((6, 7))
            if follow:
                a[:, 0] = np.clip(mid[:, 0] - 0.95, -0.15, 0.15)                # the board's grips are 0.95 m from its robot-side edge
                a[:, 1] = np.clip(mid[:, 1], -0.15, 0.15)
                a[:, 2] = np.clip(1.5 * mid[:, 2], -0.15, 0.15)
            obs, r, dn, info = B.step(a)
            assert not info[:, 11].any()
            held += int((B.term_obs[:, 39] != 0).sum())
            wins += int(((dn != 0) & (info[:, 9] > 0)).sum())
            fails += int(((dn != 0) & (info[:, 9] == 0)).sum())
        outcome[follow] = (wins, fails, held / (6 * 135))
        B.close()
    assert outcome[True][0] >= 6 and outcome[True][1] == 0 and outcome[True][2] > 0.9, outcome
    assert outcome[False][0] == 0 and outcome[False][1] >= 6, outcome


@pytest.mark.gpu
def test_hip_matches_oracle_through_success_and_the_next_task():
    """done_at_success=False: when the animation completes, _on_goal_reached puts the robot back to its initial posture, resets the controller / shield
    memory, starts the next animation and puts the board back into the gripper, inside the same episode."""
    from helpers import make_pair
    from parity import Run
    nominal = lifting_hands_nominal(hrg.build_model_desc(None, env_id=ENV))
    clips = hrg.synthetic_clips(3, fps=20.0, lifting=nominal, lift_height=0.1, min_frames=20, max_frames=26)
    O, G = make_pair(4, dict(seed=5, horizon=200, done_at_success=False, shield_type="SSM"), clips=clips, env_id=ENV)
    run = Run(O, G, "lifting through success", free_running=True, violent=None, atol=2e-6, reward_atol=2e-6)
    rng = np.random.RandomState(1)
    goals = 0
    for s in run.steps(45, lambda k: rng.uniform(-0.2, 0.2, (4, 7))):
        s.compare()
        goals = max(goals, int(s.o.info[:, 9].max()))
        if s.k % 4 == 3:
            s.resync()
    assert goals >= 2          # several tasks in a row within one episode
    run.finish()


@pytest.mark.gpu
def test_hip_matches_oracle_with_cartesian_actions_and_the_follower():
    """The IK front-end + collision prevention in front of the lifting task (config/wrappers/safe_ik.yaml), driven by the scripted follower."""
    from helpers import make_pair
    from parity import Run
    O, G = make_pair(4, dict(seed=7, horizon=200), clips=_clips(2, 100, 130), env_id=ENV, ik_position_delta=dict(action_limit=0.15),
                     collision_prevention=dict(replace_type=0, n_resamples=20))
    run = Run(O, G, "lifting follower", free_running=True, violent=None, atol=2e-6, reward_atol=2e-6, actions=(1e-6, 1e-9))
    obs = O.obs.copy()
    held = 0

    def actions(k):
        mid = 0.5 * (obs[:, 0:3] + obs[:, 4:7])
        a = np.zeros((4, 7))
        a[:, 0], a[:, 1], a[:, 2] = np.clip(mid[:, 0] - 0.95, -0.15, 0.15), np.clip(mid[:, 1], -0.15, 0.15), np.clip(1.5 * mid[:, 2], -0.15, 0.15)
        return a
    for s in run.steps(48, actions):
        s.compare()
        obs = s.o.obs
        held += int(s.o.term_obs[:, 39].sum())
        if s.k % 4 == 3:
            s.resync()
    assert held > 4 * 30
    run.finish()


@pytest.mark.gpu
def test_follower_succeeds_on_the_hip_stepper_end_to_end():
    """The product path alone (HipVecEnv + in-kernel IK front-end, no oracle in the loop): the scripted follower of demos/demo_lifting_follower_hip.py
    carries the board through on (nearly) every env; a resting robot never does."""
    from human_robot_gym_amd.vec_env import HipVecEnv
    clips = mixed.task_clips(ENV, 4, min_frames=200, max_frames=260)
    n = 32
    out = {}
    for follow in (True, False):
        env = HipVecEnv(n, env_id=ENV, env_kwargs=dict(seed=0, horizon=400), clips=clips, ik_position_delta=dict(action_limit=0.15),
                        obs_keys=["vec_eef_to_human_lh", "vec_eef_to_human_rh", "board_balance", "board_gripped"])
        obs = env.reset()
        wins = fails = 0
        for t in range(150):
            mid = 0.5 * (obs[:, 0:3] + obs[:, 3:6])
            a = np.zeros((n, 4))
            if follow:
                a[:, 0], a[:, 1], a[:, 2] = np.clip(mid[:, 0] - 0.95, -0.15, 0.15), np.clip(mid[:, 1], -0.15, 0.15), np.clip(1.5 * mid[:, 2], -0.15, 0.15)
            obs, rew, done, infos = env.step(a)
            assert np.isfinite(obs).all()
            for i in np.nonzero(done)[0]:
                wins, fails = wins + int(infos[i]["n_goal_reached"] > 0), fails + int(infos[i]["n_goal_reached"] == 0)
        out[follow] = (wins, fails)
        env.close()
    assert out[True][0] >= n - 3 and out[True][1] <= 3, out
    assert out[False][0] == 0 and out[False][1] >= n, out
