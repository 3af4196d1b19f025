"""Evaluation on the device (csrc/hrgym_eval.h): the episode ledger against tests/eval_ref.py on synthetic device tensors, the views the ledger kernels leave
against the buffers' view kernels, the fused deterministic actor against the learners' own forward pass and torch's action mapping, HipVecEnv.evaluate against a
host loop through env.step, and the checkpoint round trip of a learner in mid-training.  -m gpu.

Every comparison is bit for bit: what is copied is copied, the ledger's sums are double additions in step order, the views and the networks are the device
functions the reference values come from, and the action mapping is evaluated operation by operation as torch evaluates it.

Sizes: 6 envs in groups of 6 and 2 (quotas 1, 1, 1, 1, 2, 2 and 2, 3); actor tiles of 33 rows per group (the second tile holds one row) and of a single row, three
and two parameter sets, depths 1 and 3, actions of 4 and 7 values; 66 envs of horizon 6 in two groups of 33 with quotas 3 and 4."""
import numpy as np
import pytest

import eval_ref as E
import replay_ref as R
import human_robot_gym_amd as hrg
from human_robot_gym_amd import evaluation as EV
from human_robot_gym_amd._cstruct import CONST

pytestmark = pytest.mark.gpu

ACT_DIM = CONST["HRG_ACT_DIM"]
REACH_KEYS = ["object-state", "robot0_joint_pos"]   # 18 columns: a goal env's feature row has 6 + 6 + 18 values


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)


def _bounds(A):
    """Action bounds that are no powers of two (the unscaling rounds): float32, as an action space holds them."""
    return (np.linspace(-0.35, -0.15, A)).astype(np.float32), (np.linspace(0.15, 0.7, A)).astype(np.float32)


# ---- the ledger on synthetic rows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,P,N", [(6, 1, 8), (6, 3, 5)])
@pytest.mark.parametrize("rows", [None, "imit", "sir"])
def test_ledger_on_scripted_steps_is_the_reference(n, P, N, rows):
    steps = 12
    fed = list(R.scripted_steps(n, steps, 7, 3, done=E.done_pattern(n, steps, 3)))
    exports = {}
    for sync_every in (1, 7):
        ev = EV.Evaluator(EV.build_eval_desc(n, P, N, range(18), -np.ones(7), np.ones(7)))
        led = E.Ledger(n, P, N)
        assert ev.max_quota == led.targets.max() and ev.width == 18
        ev.begin(_dev(fed[0][1]))
        assert ev.remaining() == led.remaining() == N * P
        for t, (_, obs, _, rew, dn, info, imit, sir) in enumerate(fed):
            kw = {} if rows is None else dict(imit=imit) if rows == "imit" else dict(sir=sir)
            ev.step(_dev(obs), _dev(rew), _dev(dn), _dev(info), **{k: _dev(v) for k, v in kw.items()})
            led.step(rew, dn, info, **kw)
            if (t + 1) % sync_every == 0:
                assert ev.remaining() == led.remaining(), t
        assert ev.steps == steps and led.remaining() == 0 and ev.remaining() == 0
        counts, quota, records = ev.export()
        want_counts, want_records = led.records(ev.max_quota)
        np.testing.assert_array_equal(quota, led.targets)
        np.testing.assert_array_equal(counts, want_counts)
        _assert_bits(records, want_records, f"records, remaining read every {sync_every} steps")
        res = ev.result()
        assert res.episode_rewards == led.episode_rewards() and res.episode_lengths == led.episode_lengths()   # the order: by finishing step, then env
        np.testing.assert_array_equal(res.env, led.column("env"))
        np.testing.assert_array_equal(res.truncated, led.column("truncated"))
        np.testing.assert_array_equal(res.ep_im_rew, led.column("ep_im"))
        assert (res.mean_reward, res.std_reward) == led.mean_std()
        assert [p.episode_rewards for p in res.by_policy()] == [led.episode_rewards(k) for k in range(P)]
        exports[sync_every] = records
        ev.begin(_dev(fed[0][1]))   # a new evaluation on the same handle starts from nothing
        assert ev.remaining() == N * P and ev.steps == 0 and (ev.export()[0] == 0).all()
        ev.close()
    _assert_bits(exports[1], exports[7], "the ledger does not depend on how often the host reads `remaining`")


def test_abi_refusals():
    import ctypes
    from human_robot_gym_amd._lib import HrgError, load_library
    lib = load_library()
    ok = dict(obs_cols=range(18), act_low=-np.ones(7), act_high=np.ones(7))

    def create(change):
        d = EV.build_eval_desc(6, 3, 5, **ok)
        change(d)
        h = ctypes.c_void_p()
        rc = lib.hrg_eval_create(ctypes.byref(d), 0, ctypes.byref(h))
        assert rc != 0 and not h.value
        return lib.hrg_last_error().decode()

    assert "not divisible by n_policies" in create(lambda d: setattr(d, "n_envs", 7))
    assert "n_eval_episodes must be positive" in create(lambda d: setattr(d, "n_eval_episodes", 0))
    assert "HRG_EVAL_MAX_EPISODES_PER_ENV" in create(lambda d: setattr(d, "n_eval_episodes", 2 * CONST["HRG_EVAL_MAX_EPISODES_PER_ENV"] + 1))
    assert "squash needs normalize" in create(lambda d: setattr(d, "squash", 1))
    assert "goal_kind" in create(lambda d: (setattr(d, "goal_env", 1), setattr(d, "goal_kind", 5)))
    ev = EV.Evaluator(EV.build_eval_desc(6, 1, 5, range(18), -np.ones(7), np.ones(7), observe_time=True))
    with pytest.raises(ValueError, match="time column"):
        ev.begin(_dev(np.zeros((6, 64), np.float32)))
    z = np.zeros
    with pytest.raises(HrgError, match="observe_time needs the state imitation rows"):
        ev.step(_dev(z((6, 64), np.float32)), _dev(z(6, np.float32)), _dev(z(6, np.uint8)), _dev(z((6, 14), np.int32)))
    from human_robot_gym_amd.sac import SacLearner
    learner = SacLearner(18, 7, net_arch=[64], batch_size=32)
    with pytest.raises(HrgError, match="the evaluator's view has 19"):
        ev.policy(learner)
    ev.close()
    learner.close()


# ---- the views ----------------------------------------------------------------------------------------------------------------------------------------
def _feed(ev, n, seed, sir_rows=False):
    """begin and two steps on scripted rows; yields (the rows the view is of, their time values) after each."""
    fed = list(R.scripted_steps(n, 3, 7, seed))
    time0 = np.random.RandomState(seed).uniform(0, 1, n).astype(np.float32)
    ev.begin(_dev(fed[0][1]), _dev(time0) if sir_rows else None)
    yield fed[0][1], time0
    for _, obs, _, rew, dn, info, _, sir in fed[1:]:
        ev.step(_dev(obs), _dev(rew), _dev(dn), _dev(info), **(dict(sir=_dev(sir)) if sir_rows else {}))
        yield obs, sir[:, R.SIR_TIME_OBS]


@pytest.mark.parametrize("squash", [None, 0.5])
def test_view_with_obs_norm_and_the_time_column_is_hrg_replay_view(squash):
    from human_robot_gym_amd.replay import ReplayBuffer, build_replay_desc
    n, cols = 9, [int(c) for c in np.random.RandomState(5).permutation(64)[:63]]
    rng = np.random.RandomState(1)
    mean, std = rng.uniform(-1, 1, 64), rng.uniform(0.1, 10, 64)
    ev = EV.Evaluator(EV.build_eval_desc(n, 1, 4, cols, -np.ones(7), np.ones(7), observe_time=True, mean=mean, std=std, squash_factor=squash))
    rb = ReplayBuffer(build_replay_desc(n, n, cols, observe_time=True, mean=mean, std=std, squash_factor=squash))
    assert ev.width == 64
    for rows, time in _feed(ev, n, 2, sir_rows=True):
        want = rb.view(_dev(rows), _dev(np.ascontiguousarray(time, np.float32)))
        _assert_bits(ev.view.cpu().numpy(), want.cpu().numpy(), "normalised view")
        assert np.isfinite(want.cpu().numpy()).all() and (want[:, -1].cpu().numpy() != 0).any()
    ev.close()
    rb.close()


@pytest.mark.parametrize("kind", ["reach", "cube"])
def test_view_of_a_goal_env_is_hrg_her_features(kind):
    from human_robot_gym_amd.her import HerBuffer, build_her_desc
    n, cols, A = 9, [int(c) for c in np.random.RandomState(6).permutation(64)[:18]], 7 if kind == "reach" else 4
    ev = EV.Evaluator(EV.build_eval_desc(n, 3, 4, cols, -np.ones(A), np.ones(A), goal_kind=kind))
    hb = HerBuffer(build_her_desc(n, 8, 4, kind, cols, act_dim=A, goal_dist=0.1, task_reward=1.0, reward_scale=1.0))
    assert ev.width == hb.obs_features == (30 if kind == "reach" else 28)
    for rows, _ in _feed(ev, n, 4):
        _assert_bits(ev.view.cpu().numpy(), hb.observation(_dev(rows)).cpu().numpy(), "feature row")
    ev.close()
    hb.close()


def test_plain_view_is_the_column_selection():
    n, cols = 9, [int(c) for c in np.random.RandomState(7).permutation(64)[:11]]
    ev = EV.Evaluator(EV.build_eval_desc(n, 1, 4, cols, -np.ones(7), np.ones(7)))
    for rows, _ in _feed(ev, n, 5):
        _assert_bits(ev.view.cpu().numpy(), rows[:, cols], "selected columns")
    ev.close()


# ---- the fused actor ------------------------------------------------------------------------------------------------------------------------------------
def _stacked(learner, P, seed):
    """P parameter sets of the learner's shapes: its own and perturbed copies."""
    import torch
    g = torch.Generator().manual_seed(seed)
    base = learner.p.params.detach().cpu()
    return torch.stack([base + (0.3 * k) * (torch.rand(base.shape, generator=g) - 0.5) for k in range(P)]).cuda().contiguous()


@pytest.mark.parametrize("kind,depth,A,m,P", [("sac", 1, 4, 33, 3), ("sac", 3, 7, 33, 3), ("sac", 3, 7, 1, 2), ("ppo", 1, 4, 33, 3), ("ppo", 3, 7, 33, 3), ("ppo", 3, 4, 1, 2)])
def test_fused_actor_is_the_learners_forward_pass_and_torchs_mapping(kind, depth, A, m, P):
    import torch
    from human_robot_gym_amd.ppo import PpoLearner
    from human_robot_gym_amd.sac import SacLearner
    K, n = 18, m * P
    low32, high32 = _bounds(A)
    if kind == "ppo":
        low32, high32 = low32 * np.float32(0.2), high32 * np.float32(0.2)   # narrow enough that the clamp cuts some of the means
    ev = EV.Evaluator(EV.build_eval_desc(n, P, 1, range(K), low32, high32))
    if kind == "sac":
        learner = SacLearner(K, A, net_arch=[64] * depth, batch_size=32, seed=3)
    else:
        learner = PpoLearner(K, A, net_arch=[dict(pi=[64] * depth, vf=[64] * depth)] if depth == 3 else [64] * depth, batch_size=32, ortho_init=False, seed=3)
    stacked = _stacked(learner, P, 8)
    ev.view.copy_(_dev(np.random.RandomState(2).uniform(-1, 1, (n, K)).astype(np.float32)))
    ev.actions.fill_(7.0)   # every entry is written
    got = ev.policy(learner, stacked).cpu().numpy()
    own = learner.p.params.clone()
    want = torch.zeros(n, ACT_DIM, dtype=torch.float64, device="cuda")
    for k in range(P):
        learner.p.params.copy_(stacked[k])
        rows = ev.view[k * m:(k + 1) * m].contiguous()
        if kind == "sac":   # HipVecEnv.collect_steps: SB3's unscale_action in float64
            low, high = _dev(low32.astype(np.float64)), _dev(high32.astype(np.float64))
            a = learner.act(rows, deterministic=True)
            want[k * m:(k + 1) * m, :A] = low + 0.5 * (a.to(torch.float64) + 1.0) * (high - low)
        else:               # HipVecEnv.collect_rollout: the clip to the bounds in float32
            a = learner.policy(rows, deterministic=True)[0]
            want[k * m:(k + 1) * m, :A] = torch.clamp(a, _dev(low32), _dev(high32))
    learner.p.params.copy_(own)
    want = want.cpu().numpy()
    _assert_bits(got, want, f"{kind} actions")
    assert (got[:, A:] == 0).all() and np.isfinite(got).all()
    inside = (got[:, :A] > low32) & (got[:, :A] < high32)
    assert inside.any() and (kind == "sac" or m == 1 or (~inside).any())
    if P > 1:
        assert not np.array_equal(got[:m], got[m:2 * m])   # the groups run different parameters
    one = EV.Evaluator(EV.build_eval_desc(m, 1, 1, range(K), low32, high32))   # a learner alone: its own parameters
    one.view.copy_(ev.view[:m])
    _assert_bits(one.policy(learner).cpu().numpy(), got[:m], "the learner's own parameters are parameter set 0")
    for h in (one, ev, learner):
        h.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------------------
def _env_case(name):
    clips = hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300)
    kw = dict(env_kwargs=dict(horizon=6, seed=11, shield_type="OFF", reward_shaping=True), clips=clips)   # the dense reward: returns that depend on the actions
    if name == "goal":
        kw.update(goal_env=True, obs_keys=REACH_KEYS)
    if name == "norm-imitation":
        rng = np.random.RandomState(3)
        kw.update(expert=dict(id="ReachHuman"), imitation_reward=dict(alpha=0.25), obs_norm=dict(mean=rng.uniform(-0.5, 0.5, 18), std=rng.uniform(0.1, 10, 18), squash_factor=0.6),
                  obs_keys=REACH_KEYS)
    return kw


def _viewer(env, name):
    """rows of the superset (device) -> the policy's view, through the buffers' own view kernels (the views' tests pin the evaluator's to them)."""
    n = env.num_envs
    if name == "goal":
        from human_robot_gym_amd.her import HerBuffer
        hb = HerBuffer(env._her_desc(n, buffer_size=8, n_sampled_goal=4, goal_selection_strategy="future", relabel_observation=False, seed=0))
        return hb, hb.observation
    from human_robot_gym_amd.replay import ReplayBuffer
    rb = ReplayBuffer(env._replay_desc(n, buffer_size=n, seed=0))
    return rb, rb.view


def _host_eval(env, name, learner, stacked, N, plain_env=None):
    """SB3's evaluate_policy through env.step: per group the unfused `act` with the group's parameters and collect_steps's torch unscaling (PPO: `policy` and
    collect_rollout's clamp), the ledger of eval_ref fed from what step returns.  `plain_env`: an env of the same seed without the imitation reward, stepped with the same actions.  Returns (the ledger,
    the return of every appended episode summed from the rewards step handed out, the same from plain_env's rewards)."""
    import torch
    n, P, A, keys, be = env.num_envs, int(stacked.shape[0]), learner.act_dim, env._info_keys, env._backend
    m = n // P
    led = E.Ledger(n, P, N)
    buf, view = _viewer(env, name)
    low, high = (_dev(np.asarray(x, np.float64)) for x in (env.action_space.low, env.action_space.high))
    saved = learner.p.params.clone()
    env.reset()
    combined, running, own, own_running = [], np.zeros(n), [], np.zeros(n)
    if plain_env is not None:
        plain_env.reset()
    for _ in range(led.targets.max() * env.horizon):
        rows = view(_dev(env._last_full))
        act = np.zeros((n, ACT_DIM))
        for k in range(P):
            learner.p.params.copy_(stacked[k])
            part = rows[k * m:(k + 1) * m].contiguous()
            if learner._prefix == "hrg_sac":   # collect_steps's mapping
                a = learner.act(part, deterministic=True)
                act[k * m:(k + 1) * m, :A] = (low + 0.5 * (a.to(torch.float64) + 1.0) * (high - low)).cpu().numpy()
            else:                              # collect_rollout's
                a = learner.policy(part, deterministic=True)[0]
                act[k * m:(k + 1) * m, :A] = torch.clamp(a, low.float(), high.float()).cpu().numpy()
        _, rew, done, infos = env.step(act)
        info = np.zeros((n, E.INFO_DIM), np.int32)
        for i in np.nonzero(done)[0]:
            info[i] = [int(infos[i].get(k, False)) for k in keys]
        running += rew
        if plain_env is not None:
            _, plain_rew, plain_done, _ = plain_env.step(act)
            np.testing.assert_array_equal(plain_done, done)
            own_running += plain_rew
        before = len(led.episodes)
        led.step(rew, done, info, **(dict(imit=np.array(be.imit, copy=True)) if env._imit_alpha is not None else {}))
        combined += [running[e["env"]] for e in led.episodes[before:]]
        own += [own_running[e["env"]] for e in led.episodes[before:]]
        running[done] = 0
        own_running[done] = 0
        if led.remaining() == 0:
            break
    learner.p.params.copy_(saved)
    buf.close()
    return led, combined, own


@pytest.mark.parametrize("name", ["reach", "goal", "norm-imitation", "ppo"])
def test_evaluate_is_the_host_loop(name):
    """Two identically seeded envs of 66: env.evaluate with two parameter sets (the learner's and a perturbed copy), 100 episodes each, against the host loop.
    reach: flat observations; goal: goal_env=True, the feature row; norm-imitation: a squashed obs_norm and the action imitation reward; ppo: a PpoLearner."""
    from human_robot_gym_amd.ppo import PpoLearner
    from human_robot_gym_amd.sac import SacLearner
    n, P, N = 66, 2, 100
    kw = _env_case(name)
    dev_env, host_env = hrg.HipVecEnv(n, **kw), hrg.HipVecEnv(n, **kw)
    K = 30 if name == "goal" else 18
    if name == "ppo":
        learner = PpoLearner(K, 7, net_arch=[64, 64], batch_size=32, ortho_init=False, log_std_init=-1.0, seed=4)
    else:
        learner = SacLearner(K, 7, net_arch=[64, 64], batch_size=32, seed=4)
    stacked = _stacked(learner, P, 9)
    res = dev_env.evaluate(stacked, N, learner=learner, sync_every=7)
    plain_env = None
    if name == "norm-imitation":   # the same env without the expert and its reward: what "the env's own reward" is, independently of the imitation rows
        plain_env = hrg.HipVecEnv(n, **{k: v for k, v in kw.items() if k not in ("expert", "imitation_reward")})
    led, combined, own = _host_eval(host_env, name, learner, stacked, N, plain_env)
    assert led.remaining() == 0 and len(res.episode_rewards) == P * N
    assert res.episode_rewards == led.episode_rewards() and res.episode_lengths == led.episode_lengths()
    np.testing.assert_array_equal(res.env, led.column("env"))
    np.testing.assert_array_equal(res.step, led.column("step"))
    np.testing.assert_array_equal(res.truncated, led.column("truncated"))
    for j, k in enumerate(dev_env._info_keys):
        np.testing.assert_array_equal(res.infos[k], led.column(j), err_msg=k)
    _assert_bits(res.ep_im_rew, led.column("ep_im").astype(np.float64), "ep_im_rew")
    assert (res.mean_reward, res.std_reward) == led.mean_std() and res.std_reward > 0
    for k, part in enumerate(res.by_policy()):
        assert part.episode_rewards == led.episode_rewards(k) and (part.mean_reward, part.std_reward) == led.mean_std(k) and len(part.episode_rewards) == N
    assert res.by_policy()[0].episode_rewards != res.by_policy()[1].episode_rewards
    assert max(res.episode_lengths) <= 6 and res.truncated.any()
    if name == "norm-imitation":   # the returns are the env's own reward, not the combined one the step hands out
        assert res.episode_rewards != combined and (res.ep_im_rew != 0).any()
        assert res.episode_rewards == own
        plain_env.close()
    else:
        assert res.episode_rewards == combined and (res.ep_im_rew == 0).all()
    with pytest.raises(RuntimeError, match="step_async after evaluate"):
        dev_env.step_async(np.zeros((n, 7)))
    if name == "reach":
        # SB3's calling form, on a third env of the same seed: the same episodes, whatever the host's reading interval; one learner alone is one group
        again = hrg.HipVecEnv(n, **kw)
        other = again.evaluate(stacked, N, learner=learner, sync_every=1)
        assert other.episode_rewards == res.episode_rewards and other.episode_lengths == res.episode_lengths
        mean, std = EV.evaluate_policy(learner, again, n_eval_episodes=N)
        rewards, lengths = EV.evaluate_policy(learner, again, n_eval_episodes=N, return_episode_rewards=True)
        assert len(rewards) == len(lengths) == N and np.isfinite([mean, std]).all()
        with pytest.raises(NotImplementedError, match="deterministic=False"):
            again.evaluate(learner, N, deterministic=False)
        again.close()
    for h in (dev_env, host_env, learner):
        h.close()


def test_a_loop_after_evaluate_starts_from_a_reset():
    """evaluate steps the envs past the attached buffer.  collect_steps, evaluate, collect_steps on one env stores what a second env of the same history stores
    that takes a NEW buffer after the evaluation (attach_replay between two device loops resets the envs: both envs have been reset and stepped alike): the
    transitions, the current rows, the running returns and lengths, the episode sums."""
    from human_robot_gym_amd.sac import SacLearner
    n, first, second = 8, 5, 9
    kw = _env_case("reach")
    kept, fresh = hrg.HipVecEnv(n, **kw), hrg.HipVecEnv(n, **kw)
    learner = SacLearner(18, 7, net_arch=[64, 64], batch_size=32, seed=4)
    pol = lambda obs: learner.act(obs, deterministic=True)   # noqa: E731
    results = []
    for env in (kept, fresh):
        env.attach_replay(n * 40)
        env.collect_steps(pol, first)
        results.append(env.evaluate(learner, 2 * n))
    assert results[0].episode_rewards == results[1].episode_rewards and len(results[0].episode_rewards) == 2 * n
    kept.replay.episode_stats(clear=True)
    fresh.attach_replay(n * 40)
    kept.collect_steps(pol, second)
    fresh.collect_steps(pol, second)
    got, want = kept.replay.export(), fresh.replay.export()
    assert (got["pos"], want["pos"]) == (first + second, second)
    for k in ("observations", "next_observations", "actions", "rewards", "dones", "timeouts"):
        _assert_bits(got[k][first:first + second], want[k][:second], k)
    for k in ("cur_obs", "cur_time", "run_return", "run_length", "stats"):
        _assert_bits(got[k], want[k], k)
    assert want["dones"][:second].any() and want["stats"][:, 0].sum() >= n   # horizon 6: every env finished an episode within the 9 steps
    with pytest.raises(RuntimeError, match="step_async after collect_steps"):
        kept.step_async(np.zeros((n, 7)))
    for h in (kept, fresh, learner):
        h.close()


def test_evaluate_refuses_the_monitor_csv(tmp_path):
    env = hrg.HipVecEnv(2, env_kwargs=dict(horizon=4, seed=1), monitor_dir=str(tmp_path))
    from human_robot_gym_amd.sac import SacLearner
    learner = SacLearner(env.observation_space.shape[0], 7, net_arch=[64], batch_size=32)
    with pytest.raises(NotImplementedError, match="evaluate with monitor_dir"):
        env.evaluate(learner, 2)
    with pytest.raises(ValueError, match="learner="):
        env.evaluate(learner.p.params.view(1, -1), 2)
    env.close()
    learner.close()


# ---- checkpoints ------------------------------------------------------------------------------------------------------------------------------------------
def _sac_batches(B, K, A, count, seed):
    import torch
    from human_robot_gym_amd.replay import ReplayBufferSamples
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).cuda()   # noqa: E731
    return [(ReplayBufferSamples(u(B, K), u(B, A), u(B, K), (torch.rand(B, 1, generator=g) < 0.2).float().cuda(), u(B, 1)), torch.randn(B, A, generator=g).cuda(),
             torch.randn(B, A, generator=g).cuda()) for _ in range(count)]


def test_sac_checkpoint_continues_bit_for_bit(tmp_path):
    import torch
    from human_robot_gym_amd.sac import SacLearner
    B, K, A = 64, 11, 4
    kw = dict(net_arch=[64, 64], batch_size=B, learning_rate=5e-4, ent_coef="auto_0.2", target_update_interval=2, seed=6)
    batches, obs = _sac_batches(B, K, A, 5, 1), _dev(np.random.RandomState(0).uniform(-1, 1, (5, K)).astype(np.float32))

    def steps(learner, which):
        for i in which:   # even steps with supplied noise, odd ones with the learner's own draws (keyed by the step count)
            batch, e0, e1 = batches[i]
            learner.step(batch, *((e0, e1) if i % 2 == 0 else ()))

    whole, first = SacLearner(K, A, **kw), SacLearner(K, A, **kw)
    whole.act(obs)   # one draw each: the act counter moves too
    first.act(obs)
    steps(whole, range(5))
    steps(first, range(3))
    path = first.save(str(tmp_path / "m" / "model_3.npz"))
    second = SacLearner.load(path, device=0)
    assert second.n_updates == 3 and second.learning_rate == 5e-4 and second._sizes()[4] == 1 and (second.obs_dim, second.act_dim, second.depth, second.batch_size) == (K, A, 2, B)
    assert second.auto_ent_coef and second.desc.target_update_interval == 2 and second.desc.seed == 6
    steps(second, range(3, 5))
    for name in ("params", "adam_m", "adam_v", "target"):
        assert torch.equal(getattr(second.p, name), getattr(whole.p, name)), name
    assert second.n_updates == whole.n_updates == 5
    assert torch.equal(second.act(obs), whole.act(obs)) and not torch.equal(second.act(obs, deterministic=True), whole.act(obs))
    assert not torch.equal(first.p.params, whole.p.params)
    with pytest.raises(ValueError, match="kind = 'hrg_sac'"):
        from human_robot_gym_amd.ppo import PpoLearner
        PpoLearner.load(path, device=0)
    for h in (whole, first, second):
        h.close()


def test_ppo_checkpoint_continues_bit_for_bit(tmp_path):
    import torch
    from human_robot_gym_amd.ppo import PpoLearner
    from human_robot_gym_amd.rollout import RolloutBufferSamples
    B, K, A = 64, 11, 4
    kw = dict(net_arch=[dict(pi=[64, 64], vf=[64, 64])], batch_size=B, learning_rate=7e-5, clip_range=0.3, clip_range_vf=0.4, n_epochs=3, ent_coef=0.01, seed=6)
    g = torch.Generator().manual_seed(2)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).cuda()   # noqa: E731
    batches = [RolloutBufferSamples(u(B, K), u(B, A), u(B), u(B) - 3.0, u(B), u(B)) for _ in range(5)]
    obs = u(5, K)
    whole, first = PpoLearner(K, A, **kw), PpoLearner(K, A, **kw)
    for learner, count in ((whole, 5), (first, 3)):
        learner.policy(obs)
        for b in batches[:count]:
            learner.step(b)
    second = PpoLearner.load(first.save(str(tmp_path / "model_3.npz")), device=0)
    assert (second.n_updates, second.clip_range, second.clip_range_vf, second.n_epochs, second.separate, second.learning_rate) == (3, 0.3, 0.4, 3, True, 7e-5)
    for b in batches[3:]:
        second.step(b)
    for name in ("params", "adam_m", "adam_v"):
        assert torch.equal(getattr(second.p, name), getattr(whole.p, name)), name
    for x, y in zip(second.policy(obs), whole.policy(obs)):
        assert torch.equal(x, y)
    for h in (whole, first, second):
        h.close()
