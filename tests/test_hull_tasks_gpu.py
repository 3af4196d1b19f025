"""robot_geometry="hull" in the handover, lifting, stacking and hammering kernels (hrg_step_kernel_ho_hull, _lift_hull, _stack_hull, _hammer_hull).  -m gpu.

1. the MPR wave routine (hrg_test_hull_box_queries) against the numpy restatement (tests/hullbox_ref.py) at the extents of these tasks' boxes;
2. a hull batch of each of the five tasks is created and stepped;
3. the wiring against the unchanged oracle, which refines link x human and link x plane pairs but keeps capsules for link x object: every env-step with no (arm
   link, object box) pair near on either side is compared bit-exactly (contacts, info, done) and to RTOL (obs, reward, state, object block); hull-refined link x
   human / plane contacts occur in the handover and stacking runs (not in the lifting and hammering ones: see HULL_CONTACTS);
4. what the new pairs change, in the stacking and hammering kernels: a box inside a link's bounding capsule but clear of its hull is left alone, a box inside the
   hull gets ONE contact (stacking: it resolves; both: no simulation crash).  The C ABI reports contact PAIRS only (hrg_batch_contacts), so the normal and depth the
   step kernel wrote are not read back: for that state the kernel's own MPR routine (the test tap) is compared with tests/hullbox_ref.py instead, and the stacking
   cube's resolution checks the normal's sign.  The hammering board is not placed (it lies under the human's hands); its extents are covered by 1. and the CPU tests;
5. the steady state of the five tasks at the benchmark's batch (bench.bench_workload, its pre-roll and action pool);
6. a six-task mixed batch on hulls: each part bit-identical to its task alone.
"""
import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP library must bind to the HIP runtime torch ships)

import human_robot_gym_amd as hrg
from human_robot_gym_amd._cstruct import CONST
from human_robot_gym_amd.mixed import task_clips, task_env_kwargs
from human_robot_gym_amd.model import load_robot_hulls, robot_fk_numpy
from helpers import GEOM_BOX, NH, RTOL, link_object, make_pair, near_link_object, quat_mat
from parity import KINDS, Run, field, kind_of, read_blocks
import hullbox_ref as ref
from test_hull_box_gpu import _compare_tap, _find_placement, _link_world, _run_tap
from test_hull_tasks import TASKS, surface_queries, task_boxes

pytestmark = pytest.mark.gpu

NRCAP = CONST["HRG_NRCAP"]
GEOM_HUMAN0 = NRCAP
HG_HEAD = CONST["HRG_HG_HEAD"]


# ---------------------------------------------------------------------------------------------------------------- 1. the wave routine at these extents
def test_wave_routine_matches_the_numpy_reference_at_the_task_extents():
    """2400 queries: the seven hulls against the hammering board, handle, head and nail head, the lifting board and the stacking cube, shallow and grazing"""
    V, off = load_robot_hulls()
    queries = []
    for j, (name, bh) in enumerate(task_boxes()):
        for noise, seed in ((0.003, 40 + j), (0.0003, 60 + j)):
            queries += [(h, R, p, c, bR, bh) for h, R, p, c, bR in surface_queries(200, bh, seed, noise)]
    got = _run_tap(V, off, queries)
    pen, conv, exact = _compare_tap(V, off, queries, got)
    print(f"[hull_tasks tap] {len(queries)} queries: {pen} penetrating ({exact} on the same path to 1e-9), {conv} converged")
    assert len(queries) >= 2000 and 0.2 * len(queries) < pen < 0.9 * len(queries)


# ---------------------------------------------------------------------------------------------------------------- 2. creation
def _clips(env_id, n=3):
    return task_clips(env_id, n, min_frames=300, max_frames=600)


def _desc(env_id, kw, clips, geometry="hull"):
    return hrg.build_model_desc(dict(kw, **task_env_kwargs(env_id)), n_clips=clips.n_clips, env_id=env_id, robot_geometry=geometry)


@pytest.mark.parametrize("env_id", TASKS)
def test_hull_batch_is_created_and_steps(env_id):
    from human_robot_gym_amd._lib import HipBatch
    clips = _clips(env_id)
    G = HipBatch(_desc(env_id, dict(shield_type="SSM", horizon=50), clips), clips, 32)
    obs = G.reset()
    rng = np.random.RandomState(0)
    for _ in range(4):
        obs, r, d, info = G.step(torch.from_numpy(rng.uniform(-1, 1, (32, 7))).cuda())
    torch.cuda.synchronize()
    assert torch.isfinite(obs).all() and torch.isfinite(r).all()
    assert G.mpr_fallbacks() >= 0
    G.close()


# ---------------------------------------------------------------------------------------------------------------- 3. wiring vs the oracle
def _fold_onto_table(rng, n):
    """random small actions with the shoulder, elbow and wrist driven to their limits, each env in another combination of directions: arm links come down onto
    the table or the floor (hull-refined link x plane contacts)"""
    e = np.arange(n)
    a = rng.uniform(-0.3, 0.3, (n, 7))
    a[:, 1] = np.where(e % 2 == 0, 1.0, -1.0)
    a[:, 2] = np.where((e // 2) % 2 == 0, 0.8, -0.8)
    a[:, 3] = np.where((e // 4) % 2 == 0, 0.5, -0.5)
    return a


def _parity(env_id, shield, n, steps, fold):
    """violent here: the base rule alone.  The env-steps with an (arm link, object box) pair listed or near leave the comparison; so does, counted in `flicker` and
    bounded by the caller, an env-step whose contact list differs at agreeing floats (parity.Step.drop_flicker: the two kernels round differently, 2e-16 m measured)"""
    O, G = make_pair(n, dict(shield_type=shield, horizon=40, done_at_collision=False), task_frames=(300, 600), env_id=env_id, robot_geometry="hull")
    desc, kind = O.desc, kind_of(O.desc)
    run = Run(O, G, f"{env_id} {shield} hull", violent="base")
    rng = np.random.RandomState(4)
    t = dict(compared=0, total=0, hull_refined=0, link_object=0, flicker=0)
    for s in run.steps(steps, lambda k: _fold_onto_table(rng, n) if fold else rng.uniform(-1, 1, (n, 7))):
        po, no, pre = s.o.pairs, s.o.ncon, (s.pre_states, s.pre_objects)
        # an env that finished its episode in this step holds its reset state: its arm is checked at the step's start, with a margin for the whole step's motion
        lo = link_object(po, no) | link_object(s.g.pairs, s.g.ncon) | np.where(s.o.done == 0, near_link_object(desc, kind, *pre, s.o.states, s.o.objects),
                                                                               near_link_object(desc, kind, *pre, *pre, slack=0.15))
        s.chk &= ~lo
        s.drop_flicker()
        s.compare()
        s.resync()
        live = np.arange(po.shape[1])[None, :] < no[:, None]
        t["hull_refined"] += int((live & s.chk[:, None] & (po[:, :, 0] < NH) & (po[:, :, 1] >= GEOM_HUMAN0) & (po[:, :, 1] < GEOM_BOX)).sum())
        t["link_object"] += int(lo.sum())
        t["compared"] += int(s.chk.sum()); t["total"] += n
    t["flicker"] = run.flicker
    t["mpr_fallbacks"] = G.mpr_fallbacks()
    print(f"[hull_tasks parity] {env_id} {shield} {'fold' if fold else 'random'}: {t}")
    run.finish()
    return t


# tasks whose random / folding arms reach the human or a plane in these runs.  Not lifting: the table slab (x 0.8 .. 1.2 m) lies beyond what the arm's links reach
# with a capsule end point inside the slab's footprint and above its mid-plane (the table broadphase), and the human stands clear of the arm that hangs on the board.
# Not hammering: the folding arm meets the board first, and an arm set down onto the table below it drags the hammer in its fingers into violent motion (an
# env-step that leaves the comparison).  Their link x human / plane pairs run the collide rounds the other hull variants share (hrgym_kernels.h, robot_hulls).
HULL_CONTACTS = ("HumanRobotHandoverCart", "RobotHumanHandoverCart", "CollaborativeStackingCart")


@pytest.mark.parametrize("env_id", TASKS)
def test_hull_task_matches_the_oracle_away_from_link_object_pairs(env_id):
    shields = ("PFL", "OFF") if "Handover" in env_id else ("SSM", "OFF")
    ta = _parity(env_id, shields[0], 16, 40, False)
    tb = _parity(env_id, shields[1], 16, 40, env_id != "CollaborativeHammeringCart")   # (a folding hammering arm ends on the board: random actions there)
    for t in (ta, tb):
        assert t["compared"] >= 0.5 * t["total"], t
        assert t["flicker"] <= max(2, t["total"] // 100), t
    if env_id in HULL_CONTACTS:
        assert ta["hull_refined"] + tb["hull_refined"] > 0, (ta, tb)


# ---------------------------------------------------------------------------------------------------------------- 4. behaviour of the new pairs
def _one_env(env_id, geometry, n_cycles):
    from human_robot_gym_amd._lib import HipBatch
    clips = _clips(env_id, 1)
    d = _desc(env_id, dict(shield_type="OFF", horizon=100, done_at_collision=False), clips, geometry)
    d.n_cycles = n_cycles
    G = HipBatch(d, clips, 1)
    G.reset()
    return G, _desc(env_id, dict(shield_type="OFF", horizon=100, done_at_collision=False), clips, "capsule")


def _pairs(G):
    p, n = G.contacts()
    return [tuple(p[0, i]) for i in range(n[0])]


def _tap_contact(L, Rb, pb, c, bR, bh):
    V, off = load_robot_hulls()
    g = _run_tap(V, off, [(L, Rb, pb, c, bR, bh)])[0]
    st, depth, n, pos = ref.mpr_penetration(V[off[L]:off[L + 1]], Rb, pb, c, bR, bh)
    return g, (st, depth, n, pos)


def _place_cube(G, c, pos):
    sk = G.get_stack(0)
    sk.pos[c][:] = list(pos); sk.quat[c][:] = [1, 0, 0, 0]; sk.vel[c][:] = [0.0] * 6; sk.acc_warmstart[c][:] = [0.0] * 6; sk.obs_pos[c][:] = list(pos)
    G.set_stack(0, sk)


def test_stacking_cube_clear_of_the_hull_is_left_alone_and_inside_gets_one_contact():
    env_id = "CollaborativeStackingCart"
    G_c, desc = _one_env(env_id, "capsule", 1)
    G_h, _ = _one_env(env_id, "hull", 1)
    qpos = list(G_h.get_state(0).qpos)
    h = desc.box_half[0]
    L, c = _find_placement(desc, qpos, h, False, np.random.RandomState(2))
    a = torch.zeros((1, 7), dtype=torch.float64, device="cuda")
    for G in (G_c, G_h):
        _place_cube(G, 0, c)
        G.step(a)
    torch.cuda.synchronize()
    assert (L, GEOM_BOX) in _pairs(G_c), _pairs(G_c)          # the capsule reports the pair ...
    assert (L, GEOM_BOX) not in _pairs(G_h), _pairs(G_h)      # ... the hull does not
    G_c.close(); G_h.close()
    # inside the hull: one contact, whose MPR answer for that state is the reference's
    G1, _ = _one_env(env_id, "hull", 1)
    L, c = _find_placement(desc, qpos, h, True, np.random.RandomState(3))
    Rb, pb, *_ = _link_world(desc, qpos, L)
    _place_cube(G1, 0, c)
    G1.step(a)
    torch.cuda.synchronize()
    assert _pairs(G1).count((L, GEOM_BOX)) == 1, _pairs(G1)
    g, (st, depth, n, pos) = _tap_contact(L, Rb, pb, c, np.eye(3), np.full(3, h))
    assert st == ref.PENETRATING and g[0] == 1 and abs(g[1] - depth) <= 1e-9 and np.abs(g[2:5] - n).max() <= 1e-9, (g, depth, n)
    G1.close()
    # ... and it resolves at the normal rate, without a crash
    G, _ = _one_env(env_id, "hull", desc.n_cycles)
    _place_cube(G, 0, c)
    crash = 0
    for _ in range(3):
        _, _, _, info = G.step(a)
        crash += int(info[0, 11].item())
    torch.cuda.synchronize()
    sk = G.get_stack(0)
    Rb, pb, *_, Vb = _link_world(desc, list(G.get_state(0).qpos), L)
    st, depth, _, _ = ref.mpr_penetration(Vb, Rb, pb, np.array(sk.pos[0][:]), quat_mat(sk.quat[0][:]), np.full(3, h))
    print(f"[hull_tasks] stacking link {L}: after 3 steps depth {depth if st == ref.PENETRATING else 0.0:.2e}; crashes {crash}; fallbacks {G.mpr_fallbacks()}")
    assert (st != ref.PENETRATING or depth < 1e-3) and crash == 0, (st, depth, crash)
    G.close()


def _find_box_placement(desc, qpos, bR, bh, want_hull_hit, rng):
    """as test_hull_box_gpu._find_placement for a box of any extents and rotation: overlapping link 5's or 6's bounding capsule by >= 1 mm, clear of the hull or
    inside it by 2 .. 8 mm, clear of every other robot capsule"""
    t = np.linspace(0, 1, 200)[:, None]

    def seg_box(a, b, c):
        q = np.maximum(np.abs((a + t * (b - a) - c) @ bR) - bh, 0.0)
        return float(np.sqrt((q * q).sum(axis=1)).min())
    R, p = robot_fk_numpy(desc, np.asarray(qpos))
    caps = [(j, p[desc.rcap_body[j]] + R[desc.rcap_body[j]] @ np.array(desc.rcap_p1[j][:]), p[desc.rcap_body[j]] + R[desc.rcap_body[j]] @ np.array(desc.rcap_p2[j][:]))
            for j in range(NRCAP) if desc.rcap_body[j] >= 0]
    for L in (5, 6):
        Rb, pb, a1, a2, r, Vb = _link_world(desc, qpos, L)
        for _ in range(3000):
            u = rng.randn(3); u /= np.linalg.norm(u)
            ext = np.abs(bR.T @ u) @ bh   # the box's extent along u
            c = a1 + rng.uniform(0.1, 0.9) * (a2 - a1) + u * (r + ext - rng.uniform(0.002, 0.012))
            if seg_box(a1, a2, c) > r - 0.001:
                continue
            if any(seg_box(s1, s2, c) < desc.rcap_r[j] + 0.003 for j, s1, s2 in caps if j != L):
                continue
            st, depth, n, pos = ref.mpr_penetration(Vb, Rb, pb, c, bR, bh)
            if want_hull_hit and st == ref.PENETRATING and 0.002 <= depth <= 0.008:
                return L, c
            if not want_hull_hit and st == ref.SEPARATED:
                gap = np.maximum(np.abs((Vb @ Rb.T + pb - c) @ bR) - bh, 0.0)
                if np.sqrt((gap * gap).sum(axis=1)).min() > 0.001:
                    return L, c
    raise AssertionError("no placement found")


def test_hammer_head_clear_of_the_hull_is_left_alone_and_inside_gets_one_contact():
    """the hammer moved (its quaternion kept) so that its head sits in link 5's or 6's bounding capsule: clear of the hull no (link, head) contact, inside it one"""
    env_id = "CollaborativeHammeringCart"
    a = torch.zeros((1, 7), dtype=torch.float64, device="cuda")
    for want in (False, True):
        G_c, desc = _one_env(env_id, "capsule", 1)
        G_h, _ = _one_env(env_id, "hull", 1)
        qpos = list(G_h.get_state(0).qpos)
        hm = G_h.get_hammer(0)
        R1 = quat_mat(hm.quat[1][:])
        bh = np.array(desc.hm_geom_half[HG_HEAD][:])
        L, c = _find_box_placement(desc, qpos, R1, bh, want, np.random.RandomState(5 + want))
        for G in (G_c, G_h):
            x = G.get_hammer(0)
            x.pos[1][:] = list(c - R1 @ np.array(desc.hm_geom_pos[HG_HEAD][:])); x.vel[1][:] = [0.0] * 6
            G.set_hammer(0, x)
            G.step(a)
        torch.cuda.synchronize()
        pair = (L, GEOM_BOX + HG_HEAD)
        if not want:
            assert pair in _pairs(G_c), _pairs(G_c)
            assert pair not in _pairs(G_h), _pairs(G_h)
        else:
            assert _pairs(G_h).count(pair) == 1, _pairs(G_h)
            Rb, pb, *_ = _link_world(desc, qpos, L)
            g, (st, depth, n, pos) = _tap_contact(L, Rb, pb, c, R1, bh)
            assert st == ref.PENETRATING and g[0] == 1 and abs(g[1] - depth) <= 1e-9 and np.abs(g[2:5] - n).max() <= 1e-9, (g, depth, n)
        print(f"[hull_tasks] hammer head, link {L}, inside the hull {want}: capsule {_pairs(G_c)} hull {_pairs(G_h)}; fallbacks {G_h.mpr_fallbacks()}")
        G_c.close(); G_h.close()
        if want:   # ... the same placement stepped at the normal rate: no simulation crash, finite outputs
            G, _ = _one_env(env_id, "hull", desc.n_cycles)
            x = G.get_hammer(0)
            x.pos[1][:] = list(c - R1 @ np.array(desc.hm_geom_pos[HG_HEAD][:])); x.vel[1][:] = [0.0] * 6
            G.set_hammer(0, x)
            crash = 0
            for _ in range(3):
                obs, _, _, info = G.step(a)
                crash += int(info[0, 11].item())
            torch.cuda.synchronize()
            assert crash == 0 and torch.isfinite(obs).all(), crash
            G.close()


# ---------------------------------------------------------------------------------------------------------------- 5. steady state at the benchmark's batch
@pytest.mark.parametrize("env_id", TASKS)
def test_steady_state_at_bench_size(env_id):
    """bench.py's batch of the task (bench_workload, make_bench_batch, its action pool) with hulls against the capsule kernel on the same pool: finite outputs, no
    more simulation crashes, MPR fallbacks per env-substep below 1e-4, and oracle parity on >= 90 % of the env-steps without an (arm link, object) pair near.
    The bench's pre-roll (one horizon, at most 1000 steps), then 2 steps compared on the first 512 envs (the oracle steps those only)."""
    import bench
    from oracle.oracle import OracleBatch
    crashes = {}
    for geom in ("capsule", "hull"):
        W = bench.bench_workload(env_id, "SSM", robot_geometry=geom)
        G, desc, _, _ = bench.make_bench_batch(W)
        n = W["n"]
        pool = bench.bench_action_pool(n, G.device)
        pre = bench.bench_preroll_steps(desc)
        crash = torch.zeros((), dtype=torch.int64, device=G.device)
        for k in range(pre):
            G.step(pool[k % len(pool)])
            crash += (G.info[:, 11] != 0).sum()
        torch.cuda.synchronize()
        crashes[geom] = int(crash.item())
        for x in (G.obs, G.reward, G.term_obs):
            assert torch.isfinite(x).all(), geom
        if geom == "capsule":
            G.close()
            continue
        fb = G.mpr_fallbacks()
        rate = fb / (pre * n * desc.n_cycles)
        clips = bench._bench_clips(env_id, 0)
        m = 512
        envs = np.arange(m)
        O = OracleBatch(hrg.build_model_desc(W["env_kwargs"], n_clips=clips.n_clips, env_id=env_id, **W["wrappers"]), clips, m, env_id0=0)
        kind = kind_of(desc)
        get, put = KINDS[kind]["get"], KINDS[kind]["set"]
        for e in envs:
            O.set_state(int(e), G.get_state(int(e)))
            getattr(O, put)(int(e), getattr(G, get)(int(e)))
        good = tot = lo_n = 0
        for k in range(2):
            a = pool[(pre + k) % len(pool)]
            pre_s, pre_o = read_blocks(O, kind)
            G.step(a)
            o_o, r_o, d_o, i_o = O.step_parallel(np.ascontiguousarray(a.cpu().numpy()[:m]), n_workers=16)
            torch.cuda.synchronize()
            post_s, post_o = read_blocks(O, kind)
            o_g, r_g, d_g, i_g = [x.cpu().numpy()[envs] for x in (G.obs, G.reward, G.done, G.info)]
            po, no = O.contacts()
            pg, ng = G.contacts()
            pg, ng = pg[:m], ng[:m]
            lo = link_object(po, no) | link_object(pg, ng) | (near_link_object(desc, kind, pre_s, pre_o, post_s, post_o) & (d_o == 0))
            violent = (i_o[:, 11] != 0) | (np.abs(field(post_s, "qvel")).max(axis=1) > 5.0)
            chk = ~lo & ~violent
            same = (no == ng) & np.all(po == pg, axis=(1, 2)) & np.all(i_g == i_o, axis=1) & (d_g == d_o)
            same &= np.all(np.abs(o_g - o_o) <= 1e-6 + RTOL * np.abs(o_o), axis=1) & (np.abs(r_g - r_o) <= 1e-6 + RTOL * np.abs(r_o))
            good += int((chk & same).sum()); tot += int(chk.sum()); lo_n += int(lo.sum())
            for j, e in enumerate(envs):   # the GPU's envs continue from the oracle's states
                G.set_state(int(e), post_s[j])
                getattr(G, put)(int(e), post_o[j])
        share = good / max(tot, 1)
        print(f"[hull_tasks steady] {env_id} {n} envs: crashes capsule {crashes['capsule']} hull {crashes['hull']}; MPR fallbacks {fb} over {pre} steps "
              f"({rate:.2e} per env-substep); link-object env-steps {lo_n} of {2 * m}; parity {good} / {tot} = {share:.4f}")
        O.close(); G.close()
        assert rate < 1e-4, rate
        assert share >= 0.9 and tot >= 0.3 * 2 * m, (good, tot)
    assert crashes["hull"] <= crashes["capsule"], crashes


# ---------------------------------------------------------------------------------------------------------------- 6. the mixed batch on hulls
def test_mixed_batch_on_hulls_matches_each_task_alone():
    from human_robot_gym_amd import mixed
    from human_robot_gym_amd._lib import HipBatch
    n, steps = 6 * 48, 12
    clips = {env_id: mixed.task_clips(env_id, 3) for env_id, _ in mixed.ICRA_TASKS}
    M = mixed.make_mixed_batch(n, clips=clips, seed=7, robot_geometry="hull")
    assert all(b.mpr_fallbacks() >= 0 for b in M.batches)
    alone = []
    for (env_id, kw), sl in zip(mixed.ICRA_TASKS, M.slices):
        kw = dict(task_env_kwargs(env_id), **kw, seed=7)
        alone.append(HipBatch(hrg.build_model_desc(kw, n_clips=clips[env_id].n_clips, env_id=env_id, robot_geometry="hull"), clips[env_id], sl.stop - sl.start,
                              env_id0=sl.start))
    obs = M.reset().cpu().numpy()
    for B, sl in zip(alone, M.slices):
        np.testing.assert_array_equal(B.reset().cpu().numpy(), obs[sl.start:sl.stop])
    rng = np.random.RandomState(3)
    for k in range(steps):
        a = torch.from_numpy(rng.uniform(-1, 1, (n, 7))).cuda()
        o, r, d, i = (x.cpu().numpy() for x in M.step(a))
        for B, sl, (env_id, _) in zip(alone, M.slices, mixed.ICRA_TASKS):
            ob, rb, db, ib = (x.cpu().numpy() for x in B.step(a[sl].contiguous()))
            for x, y in ((ob, o), (rb, r), (db, d), (ib, i)):
                np.testing.assert_array_equal(x, y[sl.start:sl.stop], err_msg=f"{env_id} step {k}")
    M.close()
    for B in alone:
        B.close()
