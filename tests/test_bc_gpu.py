"""Behaviour cloning on the device (csrc/hrgym_bc.h) against tests/bc_ref.py, the torch-autograd restatement on the CPU.  -m gpu.

The yardstick is the float32 noise floor (helpers._err): `ref64` is the restatement in float64, `ref32` the same code in float32, and for a tensor X
err(X) = max|X_dev - X_ref64| / max|X_ref64|, floor(X) the same for ref32.  One step: err <= 8 floor + 2^-22; twenty steps: err <= 8 floor20 + 2^-20.
Nothing is held against the code under test.  Every err and floor is printed before it is asserted (run with -s).

Shapes: batches of 32 (one tile) and 96 (three tiles, not a power of two), observations of 1, 18 and 64 values, actions of 1, 4 and 7, depths 1 and 3, tables
of 1 row (every index 0), 37 and 1000 rows, a SAC actor and a PPO actor with a shared and with separate trunks: eleven combinations in which every one of
those values occurs with every kind of learner (CASES; the full product would be 324 learners)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bc_ref as R
import replay_ref
import sac_ref
from helpers import _dev, _err
import human_robot_gym_amd as hrg
from human_robot_gym_amd import bc as B
from human_robot_gym_amd._cstruct import CONST, BcDesc
from human_robot_gym_amd.ppo import PpoLearner
from human_robot_gym_amd.sac import SacLearner

pytestmark = pytest.mark.gpu

LR = 1e-3
# kind, separate, obs_dim, act_dim, depth, batch, table rows
CASES = [("sac", False, 1, 1, 1, 32, 1), ("sac", False, 18, 4, 3, 96, 37), ("sac", False, 64, 7, 3, 32, 1000), ("sac", False, 18, 7, 1, 96, 1000), ("sac", False, 64, 1, 1, 96, 37),
         ("ppo", False, 1, 7, 1, 96, 37), ("ppo", False, 18, 4, 3, 32, 1000), ("ppo", False, 64, 1, 3, 96, 1),
         ("ppo", True, 1, 4, 3, 32, 37), ("ppo", True, 18, 1, 1, 96, 1), ("ppo", True, 64, 7, 3, 96, 1000)]


def _learner(kind, separate, K, A, depth, params=None, seed=1):
    if kind == "sac":
        lr = SacLearner(K, A, net_arch=[64] * depth, batch_size=32, seed=seed)
    else:
        lr = PpoLearner(K, A, net_arch=[dict(pi=[64] * depth, vf=[64] * depth)] if separate else [64] * depth, batch_size=32, seed=seed)
    if params is not None:
        lr.load_state_dict(params)
    return lr


def _groups(kind, separate):
    """The parameter groups the loss reaches, by the prefix of their names."""
    if kind == "sac":
        return (("trunk", "actor.latent_pi."), ("mean head", "actor.mu."))
    return (("trunk", "mlp_extractor.policy_net." if separate else "mlp_extractor.shared_net."), ("mean head", "action_net."))


def _reached(kind, separate, name):
    return any(name.startswith(prefix) for _, prefix in _groups(kind, separate))


def _named(flat, layout):
    return {k: flat[off:off + int(np.prod(shape))].reshape(shape) for k, (off, shape) in layout.items()}


def _flat(named, prefix):
    return np.concatenate([np.asarray(torch.as_tensor(v).detach().cpu(), np.float64).reshape(-1) for k, v in named.items() if k.startswith(prefix)])


def _state(learner):
    return {k: v.clone().cpu() for k, v in learner.state_dict().items()}


@functools.lru_cache(maxsize=None)
def _one_step(kind, separate, K, A, depth, batch, n_rows):
    """One step of ref64, ref32 and the device on the same supplied rows; computed once, shared by the tests and left unchanged."""
    seed = 1000 * K + 100 * A + 10 * depth + batch + n_rows
    p = R.make_params(kind, K, A, depth, separate, seed)
    obs, act = R.make_table(K, A, n_rows, seed)
    idx = np.random.RandomState(seed).randint(0, n_rows, batch).astype(np.int64)
    s64, s32 = R.RefState(p, kind, depth, separate, torch.float64), R.RefState(p, kind, depth, separate, torch.float32)
    o64, o32 = s64.step(obs[idx], act[idx], LR), s32.step(obs[idx], act[idx], LR)
    learner = _learner(kind, separate, K, A, depth, p)
    bc = B.BehaviourCloning(learner, B.DemoTable(_dev(obs), _dev(act), kind), batch_size=batch, learning_rate=LR, seed=3)
    before = _state(learner)
    bc.step(torch.from_numpy(idx).cuda())
    ex, diag, n_entries = bc.export(), bc.diagnostics(), bc.n_entries
    after, layout = _state(learner), dict(learner.p.layout)
    bc.close()
    learner.close()
    return dict(o64=o64, o32=o32, ex=ex, diag=diag, before=before, after=after, layout=layout, grad=_named(ex["grad"], layout), idx=idx, n_entries=n_entries)


@pytest.mark.parametrize("kind, separate, K, A, depth, batch, n_rows", CASES)
def test_one_step_predictions_loss_and_gradient(kind, separate, K, A, depth, batch, n_rows):
    c = _one_step(kind, separate, K, A, depth, batch, n_rows)
    o64, o32, ex = c["o64"], c["o32"], c["ex"]
    np.testing.assert_array_equal(ex["indices"], c["idx"])
    rows = {"predictions": (ex["predictions"], o64["pred"], o32["pred"]), "loss": ([ex["loss"]], [o64["loss"]], [o32["loss"]])}
    for g, prefix in _groups(kind, separate):
        rows["grad " + g] = (_flat(c["grad"], prefix), _flat(o64["grad"], prefix), _flat(o32["grad"], prefix))
        assert np.abs(rows["grad " + g][1]).max() > 0   # (the yardstick divides by it)
    bad = []
    for k, (dev, r64, r32) in rows.items():
        err, floor = _err(dev, r64, r32)
        print(f"[bc] {kind}{' separate' if separate else ''} K {K} A {A} depth {depth} B {batch} rows {n_rows} {k}: err {err:.2e} floor {floor:.2e} ratio {err / max(floor, 1e-300):.2f}")
        if not err <= 8 * floor + 2.0 ** -22:
            bad.append(k)
    assert not bad, bad
    assert c["diag"] == dict(loss=ex["loss"], n_updates=1, learning_rate=LR)
    assert c["n_entries"] == sum(int(np.prod(shape)) for k, (_, shape) in c["layout"].items() if _reached(kind, separate, k))


@pytest.mark.parametrize("kind, separate, K, A, depth, batch, n_rows", CASES)
def test_one_step_adam_from_the_device_gradient_and_exact_zeros(kind, separate, K, A, depth, batch, n_rows):
    c = _one_step(kind, separate, K, A, depth, batch, n_rows)
    zero_seen = 0
    for k, g in c["grad"].items():
        p0, p1 = c["before"][k].double(), c["after"][k].double()
        if not _reached(kind, separate, k):   # the loss does not reach it: no gradient, the value bit for bit
            assert not (g != 0).any() and torch.equal(c["before"][k], c["after"][k]), k
            continue
        want = p0.clone()
        upd = sac_ref.adam_update(want, torch.from_numpy(g.astype(np.float64)), torch.zeros_like(want), torch.zeros_like(want), 1, LR)
        bound = 2.0 ** -23 * want.abs() + 2.0 ** -20 * LR * torch.clamp(upd.abs(), min=1.0)
        assert bool(((p1 - want).abs() <= bound).all()), k
        zero = c["o64"]["grad"][k] == 0   # exactly zero in ref64 (SAC: the dead units): exactly zero on the device, the value unchanged
        zero_seen += int(zero.sum())
        assert bool((torch.from_numpy(g)[zero] == 0).all()) and bool((p1[zero] == p0[zero]).all()), k
    assert zero_seen > 0 or kind == "ppo"
    for k in set(c["before"]) - set(c["grad"]):   # SAC's targets
        assert torch.equal(c["before"][k], c["after"][k]), k


@pytest.mark.parametrize("kind, separate", [("sac", False), ("ppo", False), ("ppo", True)])
def test_what_must_not_move(kind, separate):
    K, A, depth = 18, 4, 2
    learner = _learner(kind, separate, K, A, depth, seed=5)
    g = torch.Generator().manual_seed(0)
    learner.p.adam_m.copy_(torch.randn(learner.p.n_params, generator=g).cuda())   # an optimiser in mid-run
    learner.p.adam_v.copy_(torch.rand(learner.p.n_params, generator=g).cuda())
    rows = _dev(torch.randn(8, K, generator=g))
    learner.act(rows) if kind == "sac" else learner.policy(rows)   # the call counter at 1
    obs, act = R.make_table(K, A, 300, seed=9)
    bc = B.BehaviourCloning(learner, B.DemoTable(_dev(obs), _dev(act), kind), batch_size=64, learning_rate=LR, seed=2)
    before, m0, v0, sizes0 = _state(learner), learner.p.adam_m.clone(), learner.p.adam_v.clone(), learner._sizes()
    bc.train(5)
    after = _state(learner)
    assert bc.n_updates == 5 and bc.diagnostics()["n_updates"] == 5
    assert torch.equal(learner.p.adam_m, m0) and torch.equal(learner.p.adam_v, v0)
    assert learner._sizes() == sizes0 and sizes0[3:5] == [0, 1] and learner.n_updates == 0
    moved = sorted(k for k in before if not torch.equal(before[k], after[k]))
    assert moved == sorted(k for k in before if _reached(kind, separate, k))   # every entry of the trunk and the mean head, and nothing else
    still = set(before) - set(moved)
    if kind == "sac":
        assert {"actor.log_std.weight", "actor.log_std.bias", "log_ent_coef", "critic.qf0.0.weight", "critic.qf1.4.bias", "critic_target.qf0.0.weight", "critic_target.qf1.4.bias"} <= still
    else:
        assert {"value_net.weight", "value_net.bias", "log_std"} <= still
        assert ("mlp_extractor.value_net.0.weight" in still) if separate else ("mlp_extractor.shared_net.0.weight" in moved)
    assert float(bc.m.abs().max()) > 0 and float(bc.v.abs().max()) > 0   # the bc handle's own moments
    bc.close()
    learner.close()


def _twenty(kind, separate, K, A, depth, batch, n_rows, seed, u01=None):
    """Twenty steps on the handle's own draws from fixed parameters and a fixed table: (the learner's state, every step's indices, ref64, ref32)."""
    p = R.make_params(kind, K, A, depth, separate, seed=7)
    obs, act = R.make_table(K, A, n_rows, seed=7)
    s64, s32 = R.RefState(p, kind, depth, separate, torch.float64), R.RefState(p, kind, depth, separate, torch.float32)
    learner = _learner(kind, separate, K, A, depth, p)
    bc = B.BehaviourCloning(learner, B.DemoTable(_dev(obs), _dev(act), kind), batch_size=batch, learning_rate=LR, seed=seed)
    drawn = []
    for step in range(20):
        bc.step()
        idx = bc.export()["indices"]
        drawn.append(idx)
        if u01 is not None:
            np.testing.assert_array_equal(idx, R.draw(u01, seed, step, batch, n_rows))
            s64.step(obs[idx], act[idx], LR, outputs=False)
            s32.step(obs[idx], act[idx], LR, outputs=False)
    state = _state(learner)
    assert bc.n_updates == 20
    bc.close()
    learner.close()
    return state, np.stack(drawn), s64, s32


@pytest.mark.parametrize("kind, separate, K, A, depth, batch, n_rows", [("sac", False, 18, 7, 3, 96, 37), ("ppo", False, 6, 4, 1, 32, 1000)])
def test_twenty_steps_on_the_handles_own_draws(oracle_lib, kind, separate, K, A, depth, batch, n_rows):
    state, drawn, s64, s32 = _twenty(kind, separate, K, A, depth, batch, n_rows, 3, oracle_lib.hrgo_test_u01)
    assert drawn.min() >= 0 and drawn.max() < n_rows and len(np.unique(drawn)) > 1
    bad = []
    for k, v in state.items():
        err, floor = _err(v, s64.p[k], s32.p[k])
        print(f"[bc] twenty steps {kind} K {K} A {A} depth {depth} B {batch} rows {n_rows} {k}: err {err:.2e} floor20 {floor:.2e}")
        if not err <= 8 * floor + 2.0 ** -20:
            bad.append(k)
    assert not bad, bad
    again, drawn_again, _, _ = _twenty(kind, separate, K, A, depth, batch, n_rows, 3)
    other, drawn_other, _, _ = _twenty(kind, separate, K, A, depth, batch, n_rows, 4)
    assert all(torch.equal(state[k], again[k]) for k in state) and np.array_equal(drawn, drawn_again)
    assert not np.array_equal(drawn, drawn_other) and any(not torch.equal(state[k], other[k]) for k in state)


@pytest.mark.parametrize("kind", ["sac", "ppo"])
def test_the_loss_falls(oracle_lib, kind):
    """A 256-row table made by a fixed random teacher of the student's shape, 200 steps at B = 32: the full-table loss after is below the loss before -- first on
    ref64 alone (the inputs are adequate), then for the device's parameters, evaluated by the float64 restatement.  A sign condition, not a number."""
    K, A, depth, batch, n_rows, steps, seed = 6, 4, 2, 32, 256, 200, 11
    teacher, student = R.make_params(kind, K, A, depth, False, seed=21), R.make_params(kind, K, A, depth, False, seed=22)
    obs, _ = R.make_table(K, A, n_rows, seed=21)
    act = R.prediction({k: torch.as_tensor(v).double() for k, v in teacher.items()}, torch.as_tensor(obs).double(), kind, depth).float().numpy()
    ref = R.RefState(student, kind, depth, False, torch.float64)
    before = ref.loss(obs, act)
    for step in range(steps):
        idx = R.draw(oracle_lib.hrgo_test_u01, seed, step, batch, n_rows)
        ref.step(obs[idx], act[idx], LR, outputs=False)
    after = ref.loss(obs, act)
    print(f"[bc] {kind} teacher: full-table loss {before:.4e} -> ref64 {after:.4e}")
    assert after < before
    learner = _learner(kind, False, K, A, depth, student)
    bc = B.BehaviourCloning(learner, B.DemoTable(_dev(obs), _dev(act), kind), batch_size=batch, learning_rate=LR, seed=seed)
    bc.train(steps)
    dev = R.RefState(_state(learner), kind, depth, False, torch.float64).loss(obs, act)
    print(f"[bc] {kind} teacher: full-table loss {before:.4e} -> device {dev:.4e}")
    assert dev < before
    bc.close()
    learner.close()


def _assert_view_close(got, want, what):
    """The view's documented tolerance against the float64 restatement (tests/test_replay_gpu.py): within one float32 ulp, fewer than 1 in 1000 different."""
    d = replay_ref.ulp_distance(got, want)
    print(f"[bc] {what}: {int((d != 0).sum())} of {d.size} normalised values differ, by at most {int(d.max())} ulp")
    assert np.isfinite(got).all() and d.max() <= 1 and (d != 0).sum() * 1000 < d.size, what


@functools.lru_cache(maxsize=None)
def _reach_dataset():
    from human_robot_gym_amd.dataset import collect_expert_dataset
    return collect_expert_dataset("ReachHuman", 8, 8, expert=dict(id="ReachHuman"), env_kwargs=dict(horizon=12, seed=3, shield_type="SSM"),
                                  clips=hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300))


@pytest.mark.parametrize("algorithm", ["sac", "ppo"])
def test_on_the_real_env(tmp_path, algorithm):
    ds = _reach_dataset()
    assert ds.n_episodes == 8 and not ds.cartesian
    rng = np.random.RandomState(0)
    norm = dict(mean=rng.uniform(-0.5, 0.5, 18), std=rng.uniform(0.5, 2.0, 18)) if algorithm == "sac" else None   # (the rollout path refuses obs_norm)
    env = hrg.HipVecEnv(8, env_kwargs=dict(horizon=12, seed=5, shield_type="SSM"), clips=hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300), obs_norm=norm)
    with pytest.raises(NotImplementedError, match="demonstrations: call attach_replay"):
        env.demonstrations(ds)
    if algorithm == "sac":
        buf, learner = env.attach_replay(8 * 16), env.attach_sac(batch_size=32)
    else:
        buf, learner = env.attach_rollout(n_steps=8), env.attach_ppo(batch_size=32, net_arch=[64, 64])
    table = env.demonstrations(ds)
    rows, _ = R.table_rows(ds.ep_offset)
    assert (table.kind, table.n_rows, table.obs_dim, table.act_dim) == (algorithm, ds.total_T, 18, 7) and len(rows) == ds.total_T
    own = buf.view(torch.from_numpy(ds.obs[rows]).cuda())
    assert torch.equal(table.observations, own)
    mean, std, _ = env._norm if norm is not None else (None, None, None)
    want_obs, want_act = R.table(ds.ep_offset, ds.obs, ds.actions, env._cols, env.action_space.low, env.action_space.high, algorithm, mean=mean, std=std)
    if norm is not None:
        _assert_view_close(table.observations.cpu().numpy(), want_obs, f"{algorithm} table")
    else:
        np.testing.assert_array_equal(table.observations.cpu().numpy(), want_obs)
    np.testing.assert_array_equal(table.actions.cpu().numpy(), want_act)
    bc = env.attach_bc(table, batch_size=32)
    assert env.bc is bc and bc.desc.seed == 5 and (bc.batch_size, bc.learning_rate) == (32, 1e-3)
    with pytest.raises(IndexError, match=f"outside the table's {ds.total_T} rows"):
        bc.step(torch.full((32,), ds.total_T, dtype=torch.int64).cuda())
    start = learner.p.params.clone()
    bc.train(3)
    diag = bc.diagnostics()
    assert diag["n_updates"] == 3 and np.isfinite(diag["loss"]) and diag["loss"] > 0 and not torch.equal(start, learner.p.params)
    bc.learning_rate = 5e-4   # rescheduled between calls
    bc.train(1)
    assert bc.diagnostics() == dict(loss=bc.export()["loss"], n_updates=4, learning_rate=5e-4)
    if algorithm == "sac":   # the learner goes on as before
        env.collect_steps(learner.act, 2)
        learner.train(env.replay, 1)
    else:
        env.collect_rollout(learner.policy, learner.value)
        learner.train(env.rollout)
    assert learner.n_updates > 0 and bool(torch.isfinite(learner.p.params).all())
    res = env.evaluate(learner, 8)
    assert len(res.episode_rewards) == 8
    path = learner.save(str(tmp_path / "model.npz"))
    loaded = type(learner).load(path)
    assert torch.equal(loaded.p.params, learner.p.params) and loaded.n_updates == learner.n_updates
    fresh = _learner(algorithm, False, 18, 7, 3 if algorithm == "sac" else 2, seed=77)
    fresh.p.adam_m.fill_(0.25)
    fresh.load_parameters(path)   # what --init-checkpoint does: the parameters alone
    assert torch.equal(fresh.p.params, learner.p.params) and fresh.n_updates == 0 and bool((fresh.p.adam_m == 0.25).all())
    if algorithm == "sac":
        assert torch.equal(fresh.p.target, learner.p.target)
    for x in (loaded, fresh):
        x.close()
    env.close()
    assert env.bc is None


def test_time_column_of_a_state_imitation_reward():
    """With a state imitation reward the policy's observation ends in the time column: row t of episode k carries t / T_k, inside the normalisation."""
    ds = _reach_dataset()
    rng = np.random.RandomState(1)
    env = hrg.HipVecEnv(8, env_kwargs=dict(horizon=12, seed=5, shield_type="SSM"), clips=hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300), dataset=ds,
                        rsi_prob=0.5, state_imitation_reward=dict(alpha=0.5), obs_norm=dict(mean=rng.uniform(-0.5, 0.5, 19), std=rng.uniform(0.5, 2.0, 19)))
    env.attach_replay(8 * 4)
    learner = env.attach_sac(batch_size=32)
    table = env.demonstrations(ds)
    rows, time = R.table_rows(ds.ep_offset)
    assert env.replay.observe_time and (table.obs_dim, learner.obs_dim) == (19, 19) and len(set(time.tolist())) > 2
    assert torch.equal(table.observations, env.replay.view(torch.from_numpy(ds.obs[rows]).cuda(), time=torch.from_numpy(time).cuda()))
    mean, std, _ = env._norm
    want_obs, _ = R.table(ds.ep_offset, ds.obs, ds.actions, env._cols, env.action_space.low, env.action_space.high, "sac", observe_time=True, mean=mean, std=std)
    _assert_view_close(table.observations.cpu().numpy(), want_obs, "table with a time column")
    np.testing.assert_array_equal(want_obs[:, -1], ((time.astype(np.float64) - mean[-1]) / std[-1]).astype(np.float32))
    env.attach_bc(table, batch_size=32).train(2)
    env.collect_steps(learner.act, 2)
    assert env.bc.n_updates == 2 and bool(torch.isfinite(learner.p.params).all())
    env.close()


def test_the_library_refuses():
    """The ABI through ctypes: each refusal with its status code and message, before anything is launched."""
    learner = _learner("sac", False, 6, 4, 2)
    lib, vp = learner.lib, ctypes.c_void_p
    err = lambda: lib.hrg_last_error().decode()   # noqa: E731

    def create(entry, handle, kind=CONST["HRG_BC_SAC"], batch_size=32, device=0):
        d, out = BcDesc(), vp()
        d.kind, d.batch_size, d.seed = kind, batch_size, 1
        return getattr(lib, entry)(ctypes.byref(d), handle, device, ctypes.byref(out)), out

    for batch_size, what in ((40, "bc: batch_size = 40 is not a multiple of 32 in 32 .. 256"), (0, "bc: batch_size = 0"), (288, "bc: batch_size = 288 is not a multiple of 32 in 32 .. 256")):
        rc, out = create("hrg_bc_create_sac", learner.h, batch_size=batch_size)
        assert rc == CONST["HRG_ERR_UNSUPPORTED"] and what in err() and not out.value
    rc, out = create("hrg_bc_create_sac", learner.h, kind=CONST["HRG_BC_PPO"])
    assert rc == CONST["HRG_ERR_INVALID"] and "bc: kind = 1: this entry creates from an hrg_sac" in err() and not out.value
    rc, out = create("hrg_bc_create_sac", None)
    assert rc == CONST["HRG_ERR_INVALID"] and "null argument" in err()
    from human_robot_gym_amd.sac import SacPopulation
    pop = SacPopulation(6, 4, 2, [0, 1], net_arch=[64, 64], batch_size=32)   # a population's handle behind the entry
    rc, out = create("hrg_bc_create_sac", pop.h)
    assert rc == CONST["HRG_ERR_UNSUPPORTED"] and "bc: a population of 2 members" in err() and not out.value
    pop.close()
    rc, h = create("hrg_bc_create_sac", learner.h)
    assert rc == CONST["HRG_OK"] and h.value
    sizes = (ctypes.c_int64 * 4)()
    assert lib.hrg_bc_sizes(h, sizes) == 0 and list(sizes)[1:3] == [0, learner.p.n_params]
    obs, act, m, v = _dev(np.zeros((5, 6))), _dev(np.zeros((5, 4))), torch.zeros_like(learner.p.params), torch.zeros_like(learner.p.params)
    ptr = lambda x: vp(x.data_ptr())   # noqa: E731
    params = learner.p.params.clone()
    for args, code, what in (((None, ptr(act), 5), "HRG_ERR_INVALID", "bc: null table"), ((ptr(obs), None, 5), "HRG_ERR_INVALID", "bc: null table"),
                             ((ptr(obs), ptr(act), 0), "HRG_ERR_INVALID", "bc: n_rows = 0 must be positive"), ((ptr(obs), ptr(act), -3), "HRG_ERR_INVALID", "bc: n_rows = -3 must be positive")):
        assert lib.hrg_bc_step(h, *args, None, ptr(learner.p.params), ptr(m), ptr(v), LR, None) == CONST[code] and what in err()
    assert lib.hrg_bc_step(h, ptr(obs), ptr(act), 5, None, ptr(learner.p.params), ptr(m), ptr(v), float("nan"), None) == CONST["HRG_ERR_INVALID"] and "learning_rate" in err()
    assert lib.hrg_bc_step(h, ptr(obs), ptr(act), 5, None, None, ptr(m), ptr(v), LR, None) == CONST["HRG_ERR_INVALID"]
    assert lib.hrg_bc_sizes(h, sizes) == 0 and sizes[1] == 0   # no refused call counted as a step
    torch.cuda.synchronize()
    assert torch.equal(params, learner.p.params)
    lib.hrg_bc_destroy(h)
    learner.close()
