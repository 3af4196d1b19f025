"""Demonstration datasets on the device (csrc/hrgym_dataset.h): restore, draws, state imitation reward / early termination, accumulators and infos, the
collector, against tests/sir_ref.py and twin batches stepped with the plain hrg_batch_step.  -m gpu.

Sizes: 321 envs (one thread per env in 256-thread blocks: one full block + 65; one wavefront per env in the restore kernel), horizon 6, a dataset of three
episodes of 6, 1 and 4 transitions recorded by the collector at 8 envs."""
import ctypes
import functools

import numpy as np
import pytest

import human_robot_gym_amd as hrg
import sir_ref as R
from human_robot_gym_amd import dataset as D
from human_robot_gym_amd._cstruct import CONST, EnvState
from human_robot_gym_amd.mixed import task_clips, task_env_kwargs
from helpers import ulps32

pytestmark = pytest.mark.gpu

N, HORIZON, SEED = 321, 6, 3
IK = dict(action_limit=0.1)
EXPERTS = {"ReachHuman": dict(id="ReachHuman"), "PickPlaceHumanCart": dict(id="PickPlaceHumanCart", horizontal_epsilon=0.035),
           "CollaborativeLiftingCart": dict(id="CollaborativeLiftingCart", signal_to_noise_ratio=1.0, board_size=[1.0, 0.4, 0.03])}
KIND = {"ReachHuman": "reach", "PickPlaceHumanCart": "pick_place", "CollaborativeLiftingCart": "lifting"}
SB, BB = D.STATE_BYTES, D.BOX_BYTES
C = CONST


def _clips(env_id):
    return task_clips(env_id, 2, min_frames=200, max_frames=300)


def _env_kwargs(env_id, shield="SSM"):
    return dict(shield_type=shield, horizon=HORIZON, seed=SEED, **task_env_kwargs(env_id))


def _batch(env_id, n=N, env_id0=0, shield="SSM"):
    from human_robot_gym_amd._lib import HipBatch
    clips = _clips(env_id)
    desc = hrg.build_model_desc(_env_kwargs(env_id, shield), n_clips=clips.n_clips, env_id=env_id, ik_position_delta=None if env_id == "ReachHuman" else IK)
    return HipBatch(desc, clips, n, env_id0=env_id0)


def _collect(env_id, shield="SSM", **kw):
    return D.collect_expert_dataset(env_id, 8, 8, expert=EXPERTS[env_id], env_kwargs=_env_kwargs(env_id, shield), clips=_clips(env_id),
                                    ik_position_delta=None if env_id == "ReachHuman" else IK, **kw)


@functools.lru_cache(maxsize=None)
def _dataset(env_id):
    """Three episodes of different lengths, one with a single transition, cut from what the collector recorded at 8 envs."""
    full = _collect(env_id)
    assert full.n_episodes == 8 and full.total_T <= 8 * HORIZON and (full.boxes is None) == (env_id == "ReachHuman")
    return full.select([0, 3, 5], lengths=[min(6, full.T(0)), 1, min(4, full.T(5))])


def _bytes(arr, width):
    return np.frombuffer(arr, dtype=np.uint8).reshape(-1, width).copy()


def _states(B):
    st, bx = B.get_states(np.arange(B.n, dtype=np.int32))
    return _bytes(st, SB), _bytes(bx, BB), st, bx


def _actions(rng, env_id, n=N):
    a = np.zeros((n, 7))
    if env_id == "ReachHuman":
        a[:] = rng.uniform(-1, 1, (n, 7))
    else:
        a[:, :4] = rng.uniform([-0.1] * 3 + [-1.0], [0.1] * 3 + [1.0], (n, 4))
    return a


def _want_rows(ds, cur, restore=True):
    """Dataset bytes / observation row at the cursors `cur` [n, 3] (an env whose cursor has run to T has an observation row there and no state: its
    rows are the last state's, and no caller compares them)."""
    t = ds.ep_offset[cur[:, 0]] + cur[:, 1]
    ts = ds.ep_offset[cur[:, 0]] + np.minimum(cur[:, 1], cur[:, 2] - 1)
    return (ds.restore_states() if restore else ds.states)[ts], None if ds.boxes is None else ds.boxes[ts], ds.obs[t + cur[:, 0]]


@pytest.mark.parametrize("env_id", ["ReachHuman", "PickPlaceHumanCart"])
def test_restore_is_exact(env_id):
    """After dataset_reset and after steps whose dones are spread over the batch: a finished env's state block (and box block) equals the dataset bytes at
    its cursor bit for bit over the whole struct, its obs_dev row the dataset row; an unfinished env is exactly where a twin stepped by hrg_batch_step is."""
    import torch
    ds = _dataset(env_id)
    A, P = _batch(env_id), _batch(env_id)
    A.attach_dataset(ds, rsi_prob=1.0, seed=11)
    obs = A.dataset_reset().cpu().numpy()
    cur = A.dataset_cursor()
    s, b, _, _ = _states(A)
    ws, wb, wo = _want_rows(ds, cur)
    assert np.array_equal(s, ws) and np.array_equal(obs, wo)
    assert ds.boxes is None or np.array_equal(b, wb)
    off = EnvState.timestep.offset
    assert np.all(s[:, off:off + 4] == 0)                       # the time limit starts at zero (deviations)
    assert len(np.unique(cur[:, 0])) == 3 and cur[:, 1].max() > 0
    snap_s, snap_b = torch.empty(N, SB, dtype=torch.uint8, device="cuda"), torch.empty(N, BB, dtype=torch.uint8, device="cuda")
    A.snapshot(snap_s, None if ds.boxes is None else snap_b)    # the collector's copy is the same bytes
    assert np.array_equal(snap_s.cpu().numpy(), s) and (ds.boxes is None or np.array_equal(snap_b.cpu().numpy(), b))
    A.stagger_episode_phases(HORIZON)                           # env e is (e * 6) // 321 steps into its time limit: the dones of the next steps are spread
    _, _, st, bx = _states(A)
    P.reset()
    P.set_states(np.arange(N, dtype=np.int32), st, bx)
    rng = np.random.RandomState(0)
    alive = np.ones(N, bool)
    n_restored = 0
    for k in range(3):
        a = _actions(rng, env_id)
        prev = cur
        oa, _, da, _, _ = A.step_dataset(torch.from_numpy(a.copy()).cuda())
        op, _, dp, _ = P.step(torch.from_numpy(a.copy()).cuda())
        torch.cuda.synchronize()
        oa, da, op, dp = oa.cpu().numpy(), da.cpu().numpy() != 0, op.cpu().numpy(), dp.cpu().numpy() != 0
        cur = A.dataset_cursor()
        s, b, _, _ = _states(A)
        ps, pb, _, _ = _states(P)
        assert np.array_equal(da[alive], dp[alive]), k
        fin, un = da, alive & ~da
        ws, wb, wo = _want_rows(ds, cur)
        assert np.array_equal(s[fin], ws[fin]) and np.array_equal(oa[fin], wo[fin]), k
        assert ds.boxes is None or np.array_equal(b[fin], wb[fin]), k
        assert np.array_equal(s[un], ps[un]) and np.array_equal(b[un], pb[un]) and np.array_equal(oa[un], op[un]), k     # untouched by the restore
        assert np.array_equal(cur[~fin, 0], prev[~fin, 0]) and np.array_equal(cur[~fin, 1], np.minimum(prev[~fin, 1] + 1, prev[~fin, 2])), k
        alive &= ~da
        n_restored += int(fin.sum())
        print(f"[restore] {env_id} step {k}: {int(fin.sum())} envs restored, {int(un.sum())} compared with the twin")
    assert n_restored >= N // 3 and alive.sum() >= N // 4
    A.close(); P.close()


def test_draws(oracle_lib):
    """rsi_prob 0 / 1, cursors against the host restatement of the three draws (over the oracle's counter hash), a second (masked) reset, and a batch
    sharded 160 + 161 with the right env_id0."""
    import torch
    ds = _dataset("ReachHuman")
    Ts = np.diff(ds.ep_offset)
    assert Ts[1] == 1 and len(set(Ts.tolist())) == 3, Ts      # (6, 1, 4) unless the collector's expert ended an episode before the time limit
    u01 = oracle_lib.hrgo_test_u01
    A = _batch("ReachHuman")
    A.attach_dataset(ds, rsi_prob=0.0, seed=5)
    A.dataset_reset()
    cur = A.dataset_cursor()
    assert np.all(cur[:, 1] == 0) and np.array_equal(cur[:, 2], Ts[cur[:, 0]])
    np.testing.assert_array_equal(cur, [R.draw_cursor(u01, 5, e, 0, ds.ep_offset, 0.0) for e in range(N)])
    A.attach_dataset(ds, rsi_prob=1.0, seed=5)       # attaching again restarts the reset counters
    A.dataset_reset()
    cur = A.dataset_cursor()
    assert np.all(cur[:, 1] >= 0) and np.all(cur[:, 1] <= cur[:, 2] - 1) and np.all(cur[cur[:, 0] == 1, 1] == 0) and (cur[:, 0] == 1).sum() >= 20
    assert set(cur[cur[:, 0] == 0, 1].tolist()) == set(range(int(Ts[0])))      # every start step of the long episode is drawn
    np.testing.assert_array_equal(cur, [R.draw_cursor(u01, 5, e, 0, ds.ep_offset, 1.0) for e in range(N)])
    mask = (np.arange(N) % 3 == 0).astype(np.uint8)
    A.dataset_reset(torch.from_numpy(mask).cuda())
    cur2 = A.dataset_cursor()
    np.testing.assert_array_equal(cur2, [R.draw_cursor(u01, 5, e, 1, ds.ep_offset, 1.0) if mask[e] else tuple(cur[e]) for e in range(N)])
    A.attach_dataset(ds, rsi_prob=0.5, seed=6)
    A.dataset_reset()
    whole = A.dataset_cursor()
    A.close()
    parts = []
    for n, id0 in ((160, 0), (161, 160)):
        S = _batch("ReachHuman", n=n, env_id0=id0)
        S.attach_dataset(ds, rsi_prob=0.5, seed=6)
        S.dataset_reset()
        parts.append(S.dataset_cursor())
        S.close()
    np.testing.assert_array_equal(np.concatenate(parts), whole)
    assert 0 < (whole[:, 1] > 0).sum() < N


def _hand_made(ds, kind):
    """The recorded dataset with the `gripped` column of every second demonstration row set (pick-place, lifting): both gripped branches are met."""
    if kind == "reach":
        return ds
    obs = ds.obs.copy()
    obs[::2, R.GRIPPED] = 1.0
    obs[1::2, R.GRIPPED] = 0.0
    return D.ExpertDataset(ds.env_id, ds.ep_offset, ds.states, obs, ds.actions, boxes=ds.boxes, cartesian=ds.cartesian, obs_keys=ds.obs_keys, version=ds.version)


def _rollout(B, ds, env_id, sir, steps, seed, u01, rsi_prob=0.5, dseed=9):
    """Step `B` through hrg_batch_step_dataset and check every step against sir_ref on the rows the device itself produced.  Returns the per-step records."""
    import torch
    kind = KIND[env_id]
    p = D.sir_kwargs(env_id, sir)
    B.attach_dataset(ds, rsi_prob=rsi_prob, state_imitation_reward=sir, seed=dseed)
    B.dataset_reset()
    cur = B.dataset_cursor()
    resets = np.ones(N, np.int64)
    rng = np.random.RandomState(seed)
    acc = np.zeros((N, 6))
    out, dropped, total = [], 0, 0
    for k in range(steps):
        a = _actions(rng, env_id)
        obs, rew, done, info, srow = B.step_dataset(torch.from_numpy(a).cuda())
        torch.cuda.synchronize()
        obs, rew, done, srow, term = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy() != 0, srow.cpu().numpy(), B.term_obs.cpu().numpy()
        new = B.dataset_cursor()
        step = R.advance(cur[:, 1], cur[:, 2])
        demo = ds.obs[ds.ep_offset[cur[:, 0]] + cur[:, 0] + step]
        policy = np.where(done[:, None], term, obs)        # a finished env's own observation is its terminal one (ET alone: copied there by the restore)
        r_im, r_m, r_g, counted = R.imitation_reward(kind, demo, policy, beta=p["beta"], iota_m=p["iota_m"], iota_g=p["iota_g"], m_sim_fn=p["m_sim_fn"], g_sim_fn=p["g_sim_fn"])
        early = R.early_termination(kind, demo, policy, iota_m=p["iota_m"], et_dist=p["et_dist"]) & p["use_et"]
        ok = R.et_margin(kind, demo, policy, iota_m=p["iota_m"], et_dist=p["et_dist"]) >= 1e-9 if p["use_et"] else np.ones(N, bool)
        dropped, total = dropped + int((~ok).sum()), total + N
        r_env = srow[:, C["HRG_SIR_R_ENV"]].astype(np.float64)
        acc += np.stack([r_im, r_env, r_m, r_g, np.ones(N), counted.astype(np.float64)], axis=1)
        want = {"R_IM": r_im, "R_MOTION": r_m, "R_GRIPPER": r_g, "R_FULL": R.combine(r_im, r_env, p["alpha"]), "EP_IM": acc[:, 0], "EP_ENV": acc[:, 1], "EP_MOTION": acc[:, 2],
                "EP_GRIPPER": acc[:, 3]}
        worst = {c: float(ulps32(srow[ok, C["HRG_SIR_" + c]], w[ok]).max()) for c, w in want.items()}
        print(f"[sir] {env_id} step {k}: worst f32 ulps {worst}; early {int(early.sum())} done {int(done.sum())} mismatch {int(R.mismatch(kind, demo, policy).sum())} dropped {int((~ok).sum())}")
        msg = f"{env_id} step {k}"
        assert max(worst.values()) <= 1, msg
        assert np.array_equal(srow[:, C["HRG_SIR_R_FULL"]].view(np.uint32), rew.view(np.uint32)), msg
        assert np.array_equal(srow[ok, C["HRG_SIR_EP_LEN"]], acc[ok, 4]) and np.array_equal(srow[ok, C["HRG_SIR_EP_LEN_MG"]], acc[ok, 5]), msg
        assert np.array_equal(srow[ok, C["HRG_SIR_EARLY"]] != 0, early[ok]) and np.all(done[ok & early]), msg
        assert np.array_equal(srow[:, C["HRG_SIR_TIME"]], (step / cur[:, 2]).astype(np.float32)), msg      # one FP64 division, rounded once: exact
        fin = done
        want_cur = np.array([R.draw_cursor(u01, dseed, e, int(resets[e]), ds.ep_offset, rsi_prob) if fin[e] else (cur[e, 0], step[e], cur[e, 2]) for e in range(N)])
        np.testing.assert_array_equal(new, want_cur, err_msg=msg)       # advance, saturation at T, the draws of the restored envs
        assert np.array_equal(srow[:, C["HRG_SIR_TIME_OBS"]], (new[:, 1] / new[:, 2]).astype(np.float32)), msg
        ws, wb, wo = _want_rows(ds, new)
        assert np.array_equal(obs[fin], wo[fin]), msg
        out.append(dict(done=done, early=early, ok=ok, srow=srow, cur=cur, new=new, mismatch=R.mismatch(kind, demo, policy), dist=R.distance(kind, demo, policy)))
        acc[fin] = 0
        resets += fin
        cur = new
    assert dropped <= 0.05 * total, f"{dropped} of {total} env steps within 1e-9 of an early-termination threshold"
    return out


@pytest.mark.parametrize("env_id,fns", [("ReachHuman", ("gaussian", "tanh")), ("PickPlaceHumanCart", ("tanh", "gaussian")), ("CollaborativeLiftingCart", ("tanh", "tanh"))])
def test_reward_and_early_termination(oracle_lib, env_id, fns):
    """sir_dev against tests/sir_ref.py on the same f32 rows: rewards and episode sums within one f32 ulp (the kernel computes in FP64 and stores f32; its
    exp2 / tanh differ from numpy's by FP64 ulps, which moves the f32 rounding by one step at most); flags, done, cursor and time exact.  First without early
    termination over 8 steps (cursors saturate at T, time limits end episodes); then with it, the tolerance iota set to the median distance the first pass
    met at its first step and et_dist 1, so that both verdicts are met.

    The tanh similarity 1 - tanh(y) cancels: an FP64 ulp of tanh(y) near 1 is 1.1e-16 ABSOLUTE, and stays below a quarter of an f32 ulp of the reward only
    while the reward is above 4e-9, y < 10, distance < 18 iota.  The first pass (iota = 0.1: distances are bounded by the arm's reach, < 1.8 m) is inside that;
    the second pass, whose iota is a distance of a few centimetres, compares the motion term in its gaussian form, which has no cancellation.  (Measured with
    tanh there: CollaborativeLiftingCart, second step, 8 f32 ulps on a reward of ~1e-10 -- the two tanh implementations, not the kernel's arithmetic.)"""
    kind = KIND[env_id]
    ds = _hand_made(_dataset(env_id), kind)
    u01 = oracle_lib.hrgo_test_u01
    B = _batch(env_id)
    common = dict(alpha=0.4, use_et=False, et_dist=1.0)
    sir = dict(common, iota=0.1, sim_fn=fns[0]) if kind != "pick_place" else dict(common, beta=0.7, iota_m=0.1, iota_g=0.05, m_sim_fn=fns[0], g_sim_fn=fns[1])
    rec = _rollout(B, ds, env_id, sir, 8, 1, u01)
    assert any(r["done"].any() for r in rec) and any((r["new"][~r["done"], 1] == r["new"][~r["done"], 2]).any() for r in rec)    # restores and saturated cursors were met
    if kind == "pick_place":   # (lifting: the robot starts with the board in its gripper, so the agent's side of the mismatch comes as the random actions bring it)
        assert sum(int(r["mismatch"].sum()) for r in rec) >= 20 and sum(int((~r["mismatch"]).sum()) for r in rec) >= 20
    med = float(np.float32(np.median(rec[0]["dist"])))
    assert med > 0
    sir = dict(sir, use_et=True, **(dict(iota=med, sim_fn="gaussian") if kind != "pick_place" else dict(iota_m=med, m_sim_fn="gaussian", g_sim_fn="tanh")))
    rec = _rollout(B, ds, env_id, sir, 4, 1, u01)
    first = rec[0]
    assert (first["early"] & first["ok"]).sum() >= 20 and (~first["early"] & first["ok"]).sum() >= 20
    assert any((r["early"] & r["ok"] & r["done"]).any() for r in rec)
    B.close()


def test_alpha_zero_without_et_and_rsi_is_the_plain_step():
    """alpha = 0, use_et = False, rsi_prob = 0: rewards, dones, observations of hrg_batch_step_dataset are those of hrg_batch_step on a twin in the same
    states, bit for bit, up to and including the step at which the time limit ends the episodes."""
    import torch
    env_id = "PickPlaceHumanCart"
    ds = _dataset(env_id)
    A, P = _batch(env_id), _batch(env_id)
    A.attach_dataset(ds, rsi_prob=0.0, state_imitation_reward=dict(alpha=0.0, use_et=False, beta=0.5), seed=2)
    A.dataset_reset()
    _, _, st, bx = _states(A)
    P.reset()
    P.set_states(np.arange(N, dtype=np.int32), st, bx)
    rng = np.random.RandomState(4)
    alive = np.ones(N, bool)   # until the episode ends: then the twin starts afresh and the dataset batch from a dataset state
    for k in range(HORIZON):
        a = _actions(rng, env_id)
        ta, tp = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(a.copy()).cuda()
        oa, ra, da, ia, srow = A.step_dataset(ta)
        op, rp, dp, ip = P.step(tp)
        torch.cuda.synchronize()
        oa, ra, da, ia, srow, op, rp, dp, ip = [t.cpu().numpy() for t in (oa, ra, da, ia, srow, op, rp, dp, ip)]
        msg = f"step {k}"
        assert np.array_equal(ra.view(np.uint32)[alive], rp.view(np.uint32)[alive]), msg
        assert np.array_equal(srow[:, C["HRG_SIR_R_ENV"]].view(np.uint32)[alive], rp.view(np.uint32)[alive]), msg
        np.testing.assert_array_equal(da[alive], dp[alive], err_msg=msg)
        np.testing.assert_array_equal(ia[alive], ip[alive], err_msg=msg)
        np.testing.assert_array_equal(ta.cpu().numpy()[alive], tp.cpu().numpy()[alive], err_msg=msg)      # the executed action rows
        d = da != 0
        np.testing.assert_array_equal(oa[alive & ~d], op[alive & ~d], err_msg=msg)
        np.testing.assert_array_equal(A.term_obs.cpu().numpy()[alive & d], P.term_obs.cpu().numpy()[alive & d], err_msg=msg)
        assert not np.any(srow[:, C["HRG_SIR_EARLY"]]), msg
        print(f"[alpha 0] step {k}: {int(alive.sum())} envs compared, {int((alive & d).sum())} of them finished")
        alive &= ~d
    assert not alive.any()     # the time limit (zero at the restore) has ended every episode by now
    A.close(); P.close()


def test_infos_and_time_column_through_the_vec_env():
    """HipVecEnv(dataset=, state_imitation_reward=): the ten info keys of a done step against sums and means recomputed from the per-step rows (f32, as the host
    sees them: each term is off by half an f32 ulp at most and so is the device's rounded sum, hence the bound 2^-23 sum |term|); the pick-place means divide by
    the steps that entered the motion / gripper sums; observe_time appends step / T; early_termination sits on every info."""
    env_id = "PickPlaceHumanCart"
    ds = _hand_made(_dataset(env_id), "pick_place")
    far = ds.obs.copy()        # early termination by design: the last episode's demonstration is 100 m away (ET at its first step), every other threshold
    far[ds.obs_row0(2):, R.TO_TARGET] += 100.0       # (20 m; 2 m with a gripped mismatch) is out of reach
    ds = D.ExpertDataset(ds.env_id, ds.ep_offset, ds.states, far, ds.actions, boxes=ds.boxes, cartesian=True, obs_keys=ds.obs_keys, version=ds.version)
    sir = dict(alpha=0.4, beta=0.7, iota_m=0.05, iota_g=0.05, m_sim_fn="gaussian", g_sim_fn="tanh", observe_time=True, use_et=True, et_dist=400.0)
    env = hrg.HipVecEnv(N, env_id=env_id, env_kwargs=_env_kwargs(env_id), clips=_clips(env_id), ik_position_delta=IK, dataset=ds, rsi_prob=0.5, state_imitation_reward=sir)
    k_obs = len(env._cols)
    assert env.observation_space.shape == (k_obs + 1,) and env.observation_space.low[-1] == 0 and env.observation_space.high[-1] == 1
    assert np.all(np.isinf(env.observation_space.high[:-1]))
    obs = env.reset()
    cur = env._backend.batch.dataset_cursor()
    assert obs.shape == (N, k_obs + 1) and np.array_equal(obs[:, -1], (cur[:, 1] / cur[:, 2]).astype(np.float32))
    assert np.array_equal(obs[:, :-1], _want_rows(ds, cur)[2][:, env._cols])
    rng = np.random.RandomState(2)
    rows = [[] for _ in range(N)]
    n_done = n_early = n_partial = 0
    for k in range(8):
        obs, rew, dones, infos = env.step(rng.uniform([-0.1] * 3 + [-1.0], [0.1] * 3 + [1.0], (N, 4)))
        srow = np.array(env._backend.sir)
        new = env._backend.batch.dataset_cursor()
        step = R.advance(cur[:, 1], cur[:, 2])
        assert np.array_equal(obs[:, -1], (new[:, 1] / new[:, 2]).astype(np.float32))
        assert np.array_equal(rew, srow[:, C["HRG_SIR_R_FULL"]])
        for i in range(N):
            rows[i].append(srow[i])
            info = infos[i]
            assert info["early_termination"] == int(srow[i, C["HRG_SIR_EARLY"]])
            if not dones[i]:
                assert "ep_im_rew_mean" not in info and "terminal_observation" not in info
                continue
            r = np.array(rows[i], np.float64)
            rows[i] = []
            n_done += 1
            n_early += info["early_termination"]
            im, en, mo, gr = r[:, C["HRG_SIR_R_IM"]], r[:, C["HRG_SIR_R_ENV"]], r[:, C["HRG_SIR_R_MOTION"]], r[:, C["HRG_SIR_R_GRIPPER"]]
            counted = (mo != 0) | (gr != 0)          # a gripped-mismatch step enters neither sum (its two terms are exact zeros; a similarity never is)
            n_partial += int(0 < counted.sum() < len(r))
            tol = lambda x: 2.0 ** -23 * np.abs(x).sum() + 1e-30     # noqa: E731
            n, n_mg = len(r), int(counted.sum())
            assert info["episode"]["l"] == n and abs(info["episode"]["r"] - en.sum()) <= tol(en)
            assert abs(info["ep_im_rew_mean"] - im.sum()) <= tol(im) and abs(info["ep_env_rew_mean"] - en.sum()) <= tol(en)
            assert abs(info["ep_full_rew_mean"] - R.combine(im.sum(), en.sum(), 0.4)) <= 0.4 * tol(im) + 0.6 * tol(en)
            assert abs(info["im_rew_mean"] - im.mean()) <= tol(im) / n and abs(info["env_rew_mean"] - en.mean()) <= tol(en) / n
            assert abs(info["full_rew_mean"] - R.combine(im.mean(), en.mean(), 0.4)) <= (0.4 * tol(im) + 0.6 * tol(en)) / n
            assert abs(info["ep_m_im_rew_mean"] - mo.sum()) <= tol(mo) and abs(info["ep_g_im_rew_mean"] - gr.sum()) <= tol(gr)
            if n_mg:
                assert abs(info["m_im_rew_mean"] - mo.sum() / n_mg) <= tol(mo) / n_mg and abs(info["g_im_rew_mean"] - gr.sum() / n_mg) <= tol(gr) / n_mg
            else:
                assert np.isnan(info["m_im_rew_mean"]) and np.isnan(info["g_im_rew_mean"])
            t = info["terminal_observation"]
            assert t.shape == (k_obs + 1,) and t[-1] == np.float32(step[i] / cur[i, 2])
        cur = new
    print(f"[infos] {n_done} episodes ended, {n_early} of them early; {n_partial} with some but not all steps in the motion / gripper sums")
    assert n_done >= N and n_early >= 20 and n_done - n_early >= 20 and n_partial >= 20
    env.close()


def test_step_entries_coerce_their_actions_alike():
    """The three step entries share one routine (HipBatch._step): float64 contiguous actions and the same values as a float32, non-contiguous tensor give
    byte-identical packed blocks, imitation rows and state imitation rows through hrg_batch_step, _step_imitation and _step_dataset; a [4, 6] tensor raises
    from each of them before anything is launched (the block is untouched)."""
    import torch
    from human_robot_gym_amd._lib import HipBatch
    from human_robot_gym_amd.expert import build_expert_desc
    n, ds = 4, _dataset("ReachHuman")
    batches = []
    for _ in range(2):
        clips = _clips("ReachHuman")
        desc = hrg.build_model_desc(dict(shield_type="SSM", horizon=5, seed=SEED), n_clips=clips.n_clips, env_id="ReachHuman")
        B = HipBatch(desc, clips, n)
        B.attach_expert(build_expert_desc(dict(id="ReachHuman", seed=7), [-1.0] * 7, [1.0] * 7, dict(alpha=0.25, beta=0.7, iota_m=0.1, iota_g=0.5, m_sim_fn="gaussian", g_sim_fn="tanh")))
        B.attach_dataset(ds, rsi_prob=0.5, state_imitation_reward=dict(alpha=0.4, iota=0.1, sim_fn="gaussian"), seed=9)
        B.dataset_reset()
        batches.append(B)
    A, B = batches
    rng = np.random.RandomState(6)
    raw = lambda t: t.cpu().numpy().tobytes()      # noqa: E731
    for entry in ("step", "step_imitation", "step_dataset"):
        a32 = rng.uniform(-1, 1, (n, 7)).astype(np.float32)            # drawn as float32: the cast to float64 is exact
        wide = torch.zeros(n, 14, dtype=torch.float32, device="cuda")
        wide[:, ::2] = torch.from_numpy(a32).cuda()
        conforming, other = torch.from_numpy(a32.astype(np.float64)).cuda(), wide[:, ::2]
        assert conforming.is_contiguous() and not other.is_contiguous() and other.dtype == torch.float32
        getattr(A, entry)(conforming)
        getattr(B, entry)(other)
        torch.cuda.synchronize()
        assert raw(A.packed) == raw(B.packed) and raw(A.imit) == raw(B.imit) and raw(A.sir) == raw(B.sir), entry
        before = raw(A.packed)
        with pytest.raises(ValueError, match=r"actions must be \[4, 7\]"):
            getattr(A, entry)(torch.zeros(n, 6, dtype=torch.float64, device="cuda"))
        torch.cuda.synchronize()
        assert raw(A.packed) == before, entry
    assert np.any(A.imit.cpu().numpy() != 0) and np.any(A.sir.cpu().numpy() != 0)      # the imitation and dataset entries wrote their rows
    A.close(); B.close()


def test_collected_dataset_replays_bit_for_bit(tmp_path, monkeypatch):
    """The loop closed: collect (ReachHuman, shield off), save, load, replay every episode's recorded actions from its first recorded state: the recorded
    observation rows come back bit for bit.  Statistics files are written next to the dataset."""
    import torch
    monkeypatch.chdir(tmp_path)
    env_id = "ReachHuman"
    made = _collect(env_id, shield="OFF", dataset_name="reach-demo")
    ds = D.ExpertDataset.load("reach-demo", env_id=env_id, has_box=False)
    for key in ("ep_offset", "states", "obs", "actions"):
        assert np.array_equal(getattr(ds, key), getattr(made, key))
    assert ds.n_episodes == 8 and ds.obs_keys == ["object-state", "goal_difference"] and not ds.cartesian
    assert (tmp_path / "datasets" / "reach-demo" / "observations.csv").exists() and (tmp_path / "datasets" / "reach-demo" / "stats.csv").exists()
    from human_robot_gym_amd.training_utils import _obs_norm_from_config
    norm = _obs_norm_from_config(dict(dataset_name="reach-demo", squash_factor=None))
    np.testing.assert_allclose(norm["mean"], ds.obs[:, list(range(0, 18))].astype(np.float64).mean(axis=0), rtol=1e-15)
    n = ds.n_episodes
    B = _batch(env_id, n=n, shield="OFF")
    B.reset()
    first = ds.states[ds.ep_offset[:-1]]
    B.set_states(np.arange(n, dtype=np.int32), (EnvState * n).from_buffer_copy(first.tobytes()), None)
    T = np.diff(ds.ep_offset)
    for t in range(int(T.max())):
        live = np.nonzero(t < T)[0]
        a = np.zeros((n, 7))
        a[live] = ds.actions[ds.ep_offset[live] + t]
        obs, _, done, _ = B.step(torch.from_numpy(a).cuda())
        torch.cuda.synchronize()
        obs, term, done = obs.cpu().numpy(), B.term_obs.cpu().numpy(), done.cpu().numpy() != 0
        want = ds.obs[ds.ep_offset[live] + live + t + 1]
        last = (t + 1 == T[live])
        np.testing.assert_array_equal(done[live], last, err_msg=f"step {t}")
        got = np.where(last[:, None], term[live], obs[live])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"step {t}"
    B.close()


def test_c_abi_refusals():
    lib = _batch("ReachHuman", n=2)
    L = lib.lib
    INVALID, UNSUPPORTED = C["HRG_ERR_INVALID"], C["HRG_ERR_UNSUPPORTED"]
    ds = _dataset("ReachHuman")
    vp = ctypes.c_void_p
    import torch
    act = torch.zeros(2, 7, dtype=torch.float64, device="cuda")
    sir = torch.zeros(2, C["HRG_SIR_DIM"], dtype=torch.float32, device="cuda")
    args = lambda B, term: (B.h, vp(act.data_ptr()), vp(B.obs.data_ptr()), vp(term), vp(B.reward.data_ptr()), vp(B.done.data_ptr()), vp(B.info.data_ptr()), None,   # noqa: E731
                            vp(sir.data_ptr()), None)
    # stepping, resetting, reading the cursor without an attach
    assert L.hrg_batch_step_dataset(*args(lib, lib.term_obs.data_ptr())) == INVALID and b"no dataset attached" in L.hrg_last_error()
    assert L.hrg_batch_dataset_reset(lib.h, None, vp(lib.obs.data_ptr()), None) == INVALID
    assert L.hrg_batch_dataset_cursor(lib.h, np.zeros((2, 3), np.int32).ctypes.data_as(vp)) == INVALID
    # a sir_kind that does not fit the task
    d, keep = D.build_dataset_desc(ds, state_imitation_reward=dict(alpha=0.5))
    d.sir_kind = C["HRG_SIR_PICK_PLACE"]
    assert L.hrg_batch_dataset_attach(lib.h, ctypes.byref(d)) == UNSUPPORTED
    d.sir_kind = C["HRG_SIR_LIFTING"]
    assert L.hrg_batch_dataset_attach(lib.h, ctypes.byref(d)) == UNSUPPORTED
    # an episode with T = 0; a box array for a task without a box block
    d.sir_kind = C["HRG_SIR_REACH"]
    bad = np.array([0, 6, 6, 11], np.int64)
    d.ep_offset = bad.ctypes.data
    assert L.hrg_batch_dataset_attach(lib.h, ctypes.byref(d)) == INVALID and b"T = 0" in L.hrg_last_error()
    d.ep_offset = keep[0].ctypes.data
    d.boxes = keep[1].ctypes.data
    assert L.hrg_batch_dataset_attach(lib.h, ctypes.byref(d)) == INVALID
    d.boxes = None
    assert L.hrg_batch_dataset_attach(lib.h, ctypes.byref(d)) == 0
    # a null term_obs_dev
    assert L.hrg_batch_step_dataset(*args(lib, None)) == INVALID and b"term_obs_dev" in L.hrg_last_error()
    lib.close()
    # the stacking and hammering batches
    for env_id in ("CollaborativeStackingCart", "CollaborativeHammeringCart"):
        B = _batch(env_id, n=2)
        d, keep = D.build_dataset_desc(ds)
        assert L.hrg_batch_dataset_attach(B.h, ctypes.byref(d)) == UNSUPPORTED and b"further arrays" in L.hrg_last_error()
        st = torch.zeros(2, SB, dtype=torch.uint8, device="cuda")
        assert L.hrg_batch_snapshot(B.h, vp(st.data_ptr()), None, None) == UNSUPPORTED
        from human_robot_gym_amd._lib import HrgError
        with pytest.raises(HrgError):
            B.attach_dataset(ds)
        B.close()
