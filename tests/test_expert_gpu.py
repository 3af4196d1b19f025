"""Scripted experts + action-based imitation reward on the device (csrc/hrgym_expert.h) against tests/expert_ref.py, the recorded outputs of the
reference's expert classes (tests/golden/expert_ref.npz) and a twin batch stepped with the plain hrg_batch_step.  -m gpu.

Sizes: n_envs in {1, 65, 321}: one thread per env in 256-thread blocks, so 321 is one full block + 65 and 65 a partial block."""
import ast
import os

import numpy as np
import pytest

import human_robot_gym_amd as hrg
import expert_ref as R
from human_robot_gym_amd.expert import build_expert_desc
from human_robot_gym_amd.mixed import task_clips, task_env_kwargs
from helpers import ulps32

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "expert_ref.npz")
CART_LOW, CART_HIGH = [-0.1, -0.1, -0.1, -1.0], [0.1, 0.1, 0.1, 1.0]
JOINT_LOW, JOINT_HIGH = [-1.0] * 7, [1.0] * 7
IK = dict(action_limit=0.1)
PP_AIR = dict(hover_dist=0.2, tan_theta=0.5, horizontal_epsilon=0.035, vertical_epsilon=0.015, goal_dist=0.08, gripper_fully_opened_threshold=0.02,
              release_when_delivered=True)
REWARD = dict(alpha=0.25, beta=0.7, iota_m=0.1, iota_g=0.5, m_sim_fn="gaussian", g_sim_fn="tanh")
ATOL = 1e-12   # as test_expert.py: add, clip, sqrt, one division at magnitude <= 1 (the device's division and sqrt are good to an ulp, 2.2e-16)


@pytest.fixture(scope="module")
def fx():
    with np.load(GOLDEN) as z:
        d = {k: z[k] for k in z.files}
    d["pp_params"], d["cl_params"] = ast.literal_eval(str(d["pp_params"])), ast.literal_eval(str(d["cl_params"]))
    return d


def _batch(env_id, n, seed=3, env_id0=0, horizon=100, cp=None):
    from human_robot_gym_amd._lib import HipBatch
    clips = task_clips(env_id, 2, min_frames=200, max_frames=300)
    kw = dict(shield_type="SSM", horizon=horizon, seed=seed, **task_env_kwargs(env_id))
    desc = hrg.build_model_desc(kw, n_clips=clips.n_clips, env_id=env_id, ik_position_delta=None if env_id == "ReachHuman" else IK, collision_prevention=cp)
    return HipBatch(desc, clips, n, env_id0=env_id0)


def _desc(expert, reward=None, **kw):
    cart = expert != "ReachHuman"
    return build_expert_desc(dict(id=expert, **kw), CART_LOW if cart else JOINT_LOW, CART_HIGH if cart else JOINT_HIGH, reward)


def _fixture_obs(fx, expert, n=None):
    """Rows of the observation superset that carry the fixture inputs of `expert` in the columns it reads."""
    full = np.zeros((321, 64), np.float32)
    if expert == "ReachHuman":
        full[:, 12:18] = fx["reach_goal_difference"]
    elif expert == "PickPlaceHumanCart":
        full[:, 39] = fx["pp_object_gripped"]
        full[:, 40:43], full[:, 43:46], full[:, 53:55] = fx["pp_vec_eef_to_object"], fx["pp_vec_eef_to_target"], fx["pp_robot0_gripper_qpos"]
    elif expert == "CollaborativeLiftingCart":
        full[:, 0:3], full[:, 4:7] = fx["cl_vec_eef_to_human_lh"], fx["cl_vec_eef_to_human_rh"]
    else:
        full[:, 43:46] = fx["hm_vec_eef_to_nail"]
    return full[:n] if n else full


@pytest.mark.parametrize("expert,key,params", [("ReachHuman", "reach", {}), ("PickPlaceHumanCart", "pp", PP_AIR), ("CollaborativeLiftingCart", "cl", None),
                                               ("CollaborativeHammeringCart", "hm", {})])
def test_fixture_actions(fx, expert, key, params):
    """1. the reference's recorded actions, 321 rows per expert, through hrg_batch_expert_actions"""
    import torch
    if params is None:
        params = {k: v for k, v in fx["cl_params"].items() if k != "delta_time"}
    B = _batch(expert, 321)
    B.attach_expert(_desc(expert, signal_to_noise_ratio=1.0, **params))
    a = B.expert_actions(torch.from_numpy(_fixture_obs(fx, expert)).cuda()).cpu().numpy()
    want = fx[key + "_action"]
    w = want.shape[1]
    err = np.abs(a[:, :w] - want).max()
    print(f"[expert] {expert}: max |device - reference| = {err:.3e} over {want.size} values")
    assert err <= ATOL
    assert np.all(a[:, w:] == 0)
    B.close()


def _twin_rollout(alpha, n=65, horizon=4, steps=6):
    """PickPlaceHumanCart, Cartesian actions, collision prevention on: batch A through hrg_batch_step_imitation, twin B (same seed) through hrg_batch_step."""
    import torch
    cp = dict(replace_type=0, n_resamples=20)
    A, B = _batch("PickPlaceHumanCart", n, horizon=horizon, cp=cp), _batch("PickPlaceHumanCart", n, horizon=horizon, cp=cp)
    rw = dict(REWARD, alpha=alpha)
    A.attach_expert(_desc("PickPlaceHumanCart", rw, signal_to_noise_ratio=1.0, **PP_AIR))
    oa, ob = A.reset().cpu().numpy(), B.reset().cpu().numpy()
    np.testing.assert_array_equal(oa, ob)
    rng = np.random.RandomState(5)
    ep = np.zeros((n, 3))
    rewritten = 0
    out = []
    for k in range(steps):
        prev = A.obs.cpu().numpy().astype(np.float64)
        agent = np.zeros((n, 7))
        agent[:, :4] = rng.uniform(CART_LOW, CART_HIGH, (n, 4))
        agent[: n // 4, :4] = R.expert_from_obs("PickPlaceHumanCart", prev[: n // 4], CART_LOW, CART_HIGH, **PP_AIR) + rng.normal(0, 0.02, (n // 4, 4))   # near the expert: similarities off 0
        ta, tb = torch.from_numpy(agent.copy()).cuda(), torch.from_numpy(agent.copy()).cuda()
        o1, r1, d1, i1, imit = A.step_imitation(ta)
        o2, r2, d2, i2 = B.step(tb)
        torch.cuda.synchronize()
        o1, r1, d1, i1, imit, o2, r2, d2, i2 = [t.cpu().numpy() for t in (o1, r1, d1, i1, imit, o2, r2, d2, i2)]
        msg = f"step {k}"
        np.testing.assert_array_equal(o1, o2, err_msg=msg)
        np.testing.assert_array_equal(d1, d2, err_msg=msg)
        np.testing.assert_array_equal(i1, i2, err_msg=msg)
        np.testing.assert_array_equal(A.term_obs.cpu().numpy(), B.term_obs.cpu().numpy(), err_msg=msg)
        np.testing.assert_array_equal(ta.cpu().numpy(), tb.cpu().numpy(), err_msg=msg)   # the executed action rows
        rewritten += int(np.any(ta.cpu().numpy() != agent, axis=1).sum())
        assert np.array_equal(imit[:, 1].view(np.uint32), r2.view(np.uint32)), msg        # r_env: the twin's reward, bit for bit
        out.append(dict(prev=prev, agent=agent, r_full=r1, r_env=r2, done=d1, imit=imit))
        # expert_ref on the observation BEFORE the step and the agent's ORIGINAL action
        x = R.expert_from_obs("PickPlaceHumanCart", prev, CART_LOW, CART_HIGH, **PP_AIR)
        r_im, r_m, r_g = R.imitation_reward(agent[:, :4], x, rw["beta"], rw["iota_m"], rw["iota_g"], rw["m_sim_fn"], rw["g_sim_fn"])
        ep += np.stack([r_im, r2.astype(np.float64), np.ones(n)], axis=1)
        want = np.stack([r_im, r2.astype(np.float64), r_m, r_g, ep[:, 0], ep[:, 1], ep[:, 2], R.combine(r_im, r2.astype(np.float64), alpha)], axis=1)
        u = ulps32(imit, want)
        print(f"[imitation] alpha {alpha} {msg}: worst f32 ulps per imit column {u.max(axis=0)}; reward {ulps32(r1, want[:, 7]).max()}; done {int(d1.sum())}")
        assert u.max() <= 2 and ulps32(r1, want[:, 7]).max() <= 2, msg
        assert np.array_equal(imit[:, 7].view(np.uint32), r1.view(np.uint32)), msg
        if k == horizon - 1:
            assert np.all(d1[ep[:, 2] == horizon] != 0) and np.any(ep[:, 2] == horizon), msg   # TimeLimit: the row above carried the finished episode's sums and length
        ep[d1 != 0] = 0
    assert rewritten > 0   # the step did rewrite action rows (IK front-end): the similarities above were taken from the rows as the agent wrote them
    assert any(o["done"].any() for o in out) and np.any(out[-1]["imit"][:, 6] == steps - horizon)   # the accumulators restarted after the done step
    assert max(o["imit"][:, 2].max() for o in out) > 0.05   # some motion similarities are far from 0
    A.close(); B.close()
    return out


def test_agent_action_is_read_before_the_step_rewrites_it():
    """2. obs / done / info identical to the twin, r_env bit-equal, reward and imit row against expert_ref to 2 f32 ulps, episode sums at the done step"""
    out = _twin_rollout(alpha=0.25)
    assert any(np.any(o["r_full"] != o["r_env"]) for o in out)


def test_alpha_zero_is_the_plain_step():
    """3. alpha = 0: rewards bit-equal to hrg_batch_step's"""
    for o in _twin_rollout(alpha=0.0, steps=5):
        assert np.array_equal(o["r_full"].view(np.uint32), o["r_env"].view(np.uint32))


def test_no_noise_at_snr_one(fx):
    """4. signal_to_noise_ratio = 1: the noise state and the call counter advance and cannot be seen"""
    import torch
    for expert in ("ReachHuman", "PickPlaceHumanCart", "CollaborativeLiftingCart"):
        kw = PP_AIR if expert == "PickPlaceHumanCart" else ({k: v for k, v in fx["cl_params"].items() if k != "delta_time"} if expert == "CollaborativeLiftingCart" else {})
        B = _batch(expert, 65)
        B.attach_expert(_desc(expert, signal_to_noise_ratio=1.0, seed=1, **kw))
        obs = torch.from_numpy(_fixture_obs(fx, expert, 65)).cuda()
        first = B.expert_actions(obs).cpu().numpy().copy()
        for _ in range(3):
            np.testing.assert_array_equal(B.expert_actions(obs).cpu().numpy(), first)
        B.attach_expert(_desc(expert, signal_to_noise_ratio=1.0, seed=2, **kw))   # another seed: other draws, same actions
        np.testing.assert_array_equal(B.expert_actions(obs).cpu().numpy(), first)
        B.close()


def test_noise_is_deterministic_and_independent_of_sharding(fx):
    """5. same seed, same draws; 65 envs split 32 + 33 with env_id0 match the unsplit batch; another seed differs"""
    import torch
    obs = _fixture_obs(fx, "PickPlaceHumanCart", 65)

    def run(n, env_id0, rows, seed=11):
        B = _batch("PickPlaceHumanCart", n, env_id0=env_id0)
        B.attach_expert(_desc("PickPlaceHumanCart", signal_to_noise_ratio=0.5, seed=seed, **PP_AIR))
        t = torch.from_numpy(np.ascontiguousarray(obs[rows])).cuda()
        seq = np.stack([B.expert_actions(t).cpu().numpy().copy() for _ in range(5)])
        B.close()
        return seq
    whole = run(65, 0, slice(0, 65))
    np.testing.assert_array_equal(run(65, 0, slice(0, 65)), whole)
    np.testing.assert_array_equal(np.concatenate([run(32, 0, slice(0, 32)), run(33, 32, slice(32, 65))], axis=1), whole)
    assert np.any(whole[1] != whole[0]) and np.any(run(65, 0, slice(0, 65), seed=12) != whole)
    assert np.any(whole[0, 0, :3] != whole[0, 1, :3])   # envs draw their own noise


@pytest.mark.parametrize("expert,snr", [("ReachHuman", 0.3), ("PickPlaceHumanCart", 0.5), ("CollaborativeLiftingCart", 0.5)])
def test_noise_against_a_host_restatement(fx, oracle_lib, expert, snr):
    """6. Box-Muller over the oracle's counter hash, the recursion of expert_ref: 50 calls at the project's parity tolerance"""
    import torch
    n, seed, env_id0, dt = 65, 77, 100, 0.01
    kw = PP_AIR if expert == "PickPlaceHumanCart" else ({k: v for k, v in fx["cl_params"].items() if k != "delta_time"} if expert == "CollaborativeLiftingCart" else {})
    cart = expert != "ReachHuman"
    lo, hi = (CART_LOW, CART_HIGH) if cart else (JOINT_LOW, JOINT_HIGH)
    B = _batch(expert, n, env_id0=env_id0)
    B.attach_expert(_desc(expert, signal_to_noise_ratio=snr, seed=seed, delta_time=dt, **kw))
    full = _fixture_obs(fx, expert, n)
    obs = torch.from_numpy(full).cuda()
    alpha, sigma, dim = R.ou_params(expert, hi[0])
    y = np.zeros((n, dim))
    worst = 0.0
    for call in range(50):
        got = B.expert_actions(obs).cpu().numpy()
        xi = np.stack([R.gauss(oracle_lib.hrgo_test_u01, seed, env_id0 + e, call, dim) for e in range(n)])
        y = R.ou_step(y, xi, alpha, sigma, dt)
        want = R.expert_from_obs(expert, full, lo, hi, snr=snr, noise=y, **kw)
        worst = max(worst, np.abs(got[:, :want.shape[1]] - want).max())
        np.testing.assert_allclose(got[:, :want.shape[1]], want, rtol=1e-5, atol=1e-6, err_msg=f"call {call}")
    print(f"[noise] {expert}: max |device - host| over 50 calls = {worst:.3e}")
    assert np.abs(y).max() > 0
    B.close()


def test_noise_statistics():
    """7. reach expert (alpha 10, dt 0.01): after 400 calls the pooled variance of y over 4096 envs x 7 components is the recursion's stationary
    variance sigma^2 / (1 - alpha dt / 2) within 5 standard errors.  y is read off the action: zero goal difference and signal_to_noise_ratio 0.75 give
    a = 0.25 y (exact), clipped at |y| = 4 = 7.8 sigma, where the clip removes nothing measurable.  The last state only: successive states are correlated
    (0.9 per call), the 4096 x 7 final ones are independent draws (0.9^400 of the start is left)."""
    import torch
    n, snr, dt = 4096, 0.75, 0.01
    B = _batch("ReachHuman", n)
    B.attach_expert(_desc("ReachHuman", signal_to_noise_ratio=snr, seed=9, delta_time=dt))
    obs = torch.zeros(n, 64, dtype=torch.float32, device="cuda")
    for _ in range(400):
        a = B.expert_actions(obs)
    y = a.cpu().numpy() / (1 - snr)
    B.close()
    var = R.ou_stationary_variance(10.0, 0.5, dt)
    count = y.size
    pooled = float(np.mean(y * y))               # about the known mean 0
    se = var * np.sqrt(2.0 / count)              # standard error of the variance of `count` independent normals
    print(f"[noise] pooled variance {pooled:.6f}, stationary {var:.6f}, standard error {se:.6f} ({(pooled - var) / se:+.2f} se), mean {y.mean():+.5f}")
    assert abs(pooled - var) <= 5 * se
    assert abs(y.mean()) <= 5 * np.sqrt(var / count)
    assert np.abs(y).max() < 4.0


def _pp_env(n, horizon, **kw):
    clips = task_clips("PickPlaceHumanCart", 2, min_frames=200, max_frames=300)
    return hrg.HipVecEnv(n, env_id="PickPlaceHumanCart", env_kwargs=dict(shield_type="SSM", horizon=horizon), seed=4, clips=clips, ik_position_delta=IK,
                         expert=dict(id="PickPlaceHumanCart", signal_to_noise_ratio=1.0, **PP_AIR), **kw)


def test_vec_env_info_keys_on_done():
    """8. the six keys of _add_reward_to_info appear on done and satisfy their defining identities; Monitor's return stays the environment reward"""
    n, horizon, alpha = 65, 5, 0.25
    env = _pp_env(n, horizon, imitation_reward=dict(REWARD, alpha=alpha))
    env.reset()
    rng = np.random.RandomState(0)
    tot = np.zeros(n)
    keys = ("ep_im_rew_mean", "ep_env_rew_mean", "ep_full_rew_mean", "im_rew_mean", "env_rew_mean", "full_rew_mean")
    finished = 0
    for k in range(horizon):
        obs, rew, done, infos = env.step(rng.uniform(CART_LOW, CART_HIGH, (n, 4)))
        tot += rew
        for i in range(n):
            d = infos[i]
            if not done[i]:
                assert not any(key in d for key in keys)
                continue
            finished += 1
            length = d["episode"]["l"]
            assert all(key in d for key in keys)
            assert d["ep_full_rew_mean"] == pytest.approx(d["ep_im_rew_mean"] * alpha + d["ep_env_rew_mean"] * (1 - alpha), rel=1e-12)
            assert d["im_rew_mean"] == pytest.approx(d["ep_im_rew_mean"] / length, rel=1e-12) and d["env_rew_mean"] == pytest.approx(d["ep_env_rew_mean"] / length, rel=1e-12)
            assert d["full_rew_mean"] == pytest.approx(d["im_rew_mean"] * alpha + d["env_rew_mean"] * (1 - alpha), rel=1e-12)
            assert d["episode"]["r"] == pytest.approx(d["ep_env_rew_mean"], rel=1e-6, abs=1e-6)   # Monitor's return: the environment reward (f32 sums)
            assert tot[i] == pytest.approx(d["ep_full_rew_mean"], rel=1e-5, abs=1e-5)           # the step rewards were the combined ones
            assert 0 < d["im_rew_mean"] <= 1
            tot[i] = 0
    assert done.all() and finished >= n   # TimeLimit at the horizon
    env.close()


def test_vec_env_expert_action_shapes():
    """9. [n, 7] for the joint env, [n, 4] for a Cartesian one; n = 1"""
    clips = hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300)
    env = hrg.HipVecEnv(1, env_id="ReachHuman", env_kwargs=dict(shield_type="SSM", horizon=50), seed=1, clips=clips, expert=dict(id="ReachHuman"))
    with pytest.raises(RuntimeError):
        env.expert_actions()
    env.reset()
    a = env.expert_actions()
    assert a.shape == (1, 7) and a.dtype == np.float64
    np.testing.assert_allclose(a, R.reach(env._last_full[:, 12:18], JOINT_LOW, JOINT_HIGH), rtol=0, atol=ATOL)
    env.close()
    env = _pp_env(1, 50)
    env.reset()
    assert env.expert_actions().shape == (1, 4)
    obs, rew, done, infos = env.step(env.expert_actions())   # an expert without imitation_reward: the plain step
    assert rew.shape == (1,) and "ep_im_rew_mean" not in infos[0]
    env.close()
    plain = hrg.HipVecEnv(1, env_id="ReachHuman", env_kwargs=dict(shield_type="SSM", horizon=50), seed=1, clips=clips)
    with pytest.raises(NotImplementedError):
        plain.expert_actions()
    plain.close()


def test_mixed_vec_env_has_no_expert():
    """the mixed batch refuses: experts are per task and action form"""
    env = hrg.make_mixed_vec_env(4, tasks=[("ReachHuman", {}), ("PickPlaceHumanCart", {})], n_clips=2)
    env.reset()
    with pytest.raises(NotImplementedError, match="per task"):
        env.expert_actions()
    env.close()


def test_c_abi_refusals():
    """no expert attached: HRG_ERR_INVALID (-1); an expert that does not fit the task or the action form: HRG_ERR_UNSUPPORTED (-4)"""
    import torch
    from human_robot_gym_amd._lib import HrgError
    B = _batch("PickPlaceHumanCart", 1)
    B.reset()
    B.expert_desc, B.imit, B._expert_act = _desc("PickPlaceHumanCart"), torch.zeros(1, 8, device="cuda"), torch.zeros(1, 7, dtype=torch.float64, device="cuda")   # past the Python guard
    for call in (lambda: B.expert_actions(), lambda: B.step_imitation(torch.zeros(1, 7, dtype=torch.float64, device="cuda"))):
        with pytest.raises(HrgError, match="error -1"):
            call()
    for bad in (_desc("CollaborativeHammeringCart"), _desc("ReachHuman")):
        with pytest.raises(HrgError, match="error -4"):
            B.attach_expert(bad)
    B.attach_expert(_desc("PickPlaceHumanCart"))   # without a reward: expert actions yes, step_imitation no
    assert B.expert_actions().shape == (1, 7)
    with pytest.raises(HrgError, match="error -1"):
        B.step_imitation(torch.zeros(1, 7, dtype=torch.float64, device="cuda"))
    B.close()
    R_ = _batch("ReachHuman", 1)
    with pytest.raises(HrgError, match="error -4"):
        R_.attach_expert(_desc("PickPlaceHumanCart"))
    R_.close()


def test_vec_env_expert_drives_pick_place():
    """10. 40 steps of PickPlaceHumanCart driven by env.expert_actions(): the action sequence is expert_ref's on the returned observations"""
    n = 65
    env = _pp_env(n, 100, obs_keys=["object_gripped", "vec_eef_to_object", "vec_eef_to_target", "robot0_gripper_qpos"])
    obs = env.reset()
    gripped = 0
    for k in range(40):
        a = env.expert_actions()
        want = R.pick_place(obs[:, 0] != 0, obs[:, 1:4], obs[:, 4:7], obs[:, 7:9], 0.1, 1.0, **PP_AIR)
        np.testing.assert_allclose(a, want, rtol=0, atol=ATOL, err_msg=f"step {k}")
        obs, rew, done, infos = env.step(a)
        gripped += int((obs[:, 0] != 0).sum())
    print(f"[expert] PickPlaceHumanCart driven by its expert: {gripped} gripped env-steps of {40 * n}")
    env.close()
