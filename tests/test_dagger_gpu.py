"""DAgger on the device (csrc/hrgym_dagger.h, dagger.py, HipVecEnv.attach_dagger / collect_dagger) against tests/dagger_ref.py and against the paths that exist:
collect_steps (beta = 0), the host path driven by the expert (beta = 1).  -m gpu.

Bit for bit: the table's observations, the executed rows, PPO's labels, the kept rows of learner-driven envs, who drove, slot and n_rows.  SAC's labels (and through
them the kept rows of expert-driven envs) divide in double: the library is compiled with -fapprox-func, whose double division is a reciprocal refinement within an
ulp of the quotient in double, so the float32 label may differ from numpy's where the exact value sits next to a rounding boundary: within one
float32 ulp, fewer than 1 in 1000 different (replay_ref.ulp_distance; the counts are printed).  Statistics: 1e-12 relative."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bc_ref
import dagger_ref as R
import replay_ref
import human_robot_gym_amd as hrg
from human_robot_gym_amd import bc as B
from human_robot_gym_amd import dagger as D
from human_robot_gym_amd._cstruct import CONST, DaggerDesc
from human_robot_gym_amd.mixed import task_clips

pytestmark = pytest.mark.gpu

ACT = CONST["HRG_ACT_DIM"]
# n (6: a ragged last block of four waves; 5: two blocks), K, A, kind, the limits of the bounds
SHAPES = [(6, 19, 7, "sac", [0.1, 0.15, 0.2, 1.0, 0.1, 0.15, 1.0]), (5, 4, 4, "ppo", [0.15, 0.15, 0.15, 1.0])]
CAPACITY, STEPS, PINNED, SEED, ENV_ID0 = 3, 5, 7, 12, 100


def _clips():
    return hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300)


@functools.lru_cache(maxsize=None)
def _run(shape, beta):
    """Five steps of the handle and of the restatement on the same inputs; computed once, shared by the tests and left unchanged."""
    n, K, A, kind, limits = SHAPES[shape]
    from oracle import oracle
    u01 = oracle.load().hrgo_test_u01
    rng = np.random.RandomState(100 * shape + int(10 * beta))
    high = np.array(limits, np.float32).astype(np.float64)
    low = -high
    pinned = rng.uniform(-1, 1, (PINNED, K)).astype(np.float32), rng.uniform(-1, 1, (PINNED, A)).astype(np.float32)
    ref = R.Dagger(kind, n, K, A, CAPACITY, low, high, SEED, ENV_ID0, pinned)
    dev = D.Dagger(kind, n, K, A, CAPACITY, low, high, beta=beta, pinned=B.DemoTable(torch.from_numpy(pinned[0]).cuda(), torch.from_numpy(pinned[1]).cuda(), kind),
                   seed=SEED, env_id0=ENV_ID0)
    steps = []
    for t in range(STEPS):
        view = rng.uniform(-2, 2, (n, K)).astype(np.float32)
        learner = (rng.uniform(-1.2, 1.2, (n, A)) * (1.0 if kind == "sac" else high)).astype(np.float32)   # PPO: at the env's scale, some outside the bounds
        expert = np.zeros((n, ACT))
        expert[:, :A] = rng.uniform(-1.3, 1.3, (n, A)) * high
        expert[:, A - 1] = rng.choice([-1.0, 0.3, 1.0], n)
        expert[:, A:] = 9.0   # (columns behind A are not read)
        want = ref.step(u01, view, learner, expert, beta)
        rows = torch.full((n, ACT), 7.0, dtype=torch.float64).cuda()
        kept = torch.full((n, A), 7.0, dtype=torch.float32).cuda()
        dev.step(torch.from_numpy(view).cuda(), torch.from_numpy(learner).cuda(), torch.from_numpy(expert).cuda(), rows, kept)
        sizes = dev.sizes()
        steps.append(dict(want=want, rows=rows.cpu().numpy(), kept=kept.cpu().numpy(), sizes=sizes, n_rows=dev.table.n_rows, ref_n_rows=ref.n_rows, ref_slot=ref.slot))
    out = dict(steps=steps, obs=dev.table.observations.cpu().numpy(), act=dev.table.actions.cpu().numpy(), stats=dev.stats_per_env(clear=False), summary=dev.stats(clear=False),
               cleared=dev.stats_per_env(), after=dev.stats_per_env(), ref=ref, pinned=pinned)
    dev.close()
    return out


CASES = [(s, b) for s in range(len(SHAPES)) for b in (0.0, 0.4, 1.0)]


def _ulp_close(got, want, what):
    d = replay_ref.ulp_distance(got, want)
    print(f"[dagger] {what}: {int((d != 0).sum())} of {d.size} values differ, by at most {int(d.max()) if d.size else 0} ulp")
    assert np.isfinite(got).all() and (d.size == 0 or d.max() <= 1) and (d != 0).sum() * 1000 < max(d.size, 1), what


@pytest.mark.parametrize("shape, beta", CASES)
def test_kernel_against_the_reference(shape, beta):
    n, K, A, kind, _ = SHAPES[shape]
    c = _run(shape, beta)
    ref, drove_all = c["ref"], []
    for t, s in enumerate(c["steps"]):
        want = s["want"]
        np.testing.assert_array_equal(s["rows"], want["rows"])   # the executed rows, zeros behind A included
        drove = want["expert"]
        drove_all.append(drove)
        np.testing.assert_array_equal(s["kept"][~drove], want["kept"][~drove])   # the learner's own row
        if kind == "ppo":
            np.testing.assert_array_equal(s["kept"], want["kept"])
        else:
            _ulp_close(s["kept"][drove], want["kept"][drove], f"{kind} beta {beta} step {t}: kept rows of expert-driven envs")
        assert s["sizes"]["n_calls"] == t + 1 and s["sizes"]["slot"] == s["ref_slot"] == (t + 1) % CAPACITY
        assert s["sizes"]["n_rows"] == s["n_rows"] == s["ref_n_rows"] == PINNED + min(t + 1, CAPACITY) * n
    drove_all = np.array(drove_all)
    assert {0.0: not drove_all.any(), 1.0: drove_all.all()}.get(beta, drove_all.any() and not drove_all.all())
    np.testing.assert_array_equal(c["obs"], ref.observations)   # the view, bit for bit, in the slot's rows; the pinned rows
    if kind == "ppo":
        np.testing.assert_array_equal(c["act"], ref.actions)
    else:
        np.testing.assert_array_equal(c["act"][:PINNED], ref.actions[:PINNED])
        _ulp_close(c["act"][PINNED:], ref.actions[PINNED:], f"{kind} beta {beta}: labels")
    np.testing.assert_array_equal(c["obs"][:PINNED], c["pinned"][0])   # unchanged after the wrap
    np.testing.assert_array_equal(c["act"][:PINNED], c["pinned"][1])
    # who drove: the executed rows say it (rows == clip(expert) there), and the statistics count it
    np.testing.assert_array_equal(c["stats"][:, :2], ref.stats[:, :2])
    err = np.abs(c["stats"][:, 2] - ref.stats[:, 2]) / ref.stats[:, 2]
    print(f"[dagger] {kind} beta {beta}: squared-error sums within {err.max():.2e} relative")
    assert ref.stats[:, 2].min() > 0 and err.max() <= 1e-12
    tot = ref.stats.sum(axis=0)
    assert c["summary"]["steps"] == STEPS * n and c["summary"]["expert_steps"] == int(tot[1]) and c["summary"]["n_rows"] == PINNED + CAPACITY * n
    assert c["summary"]["imitation_error"] == pytest.approx(tot[2] / (STEPS * n * A), rel=1e-12) and c["summary"]["expert_fraction"] == tot[1] / (STEPS * n)
    np.testing.assert_array_equal(c["cleared"], c["stats"])   # the reads without clear left them; the read with clear returned them ...
    assert not c["after"].any()   # ... and zeroed them
    assert c["summary"]["beta"] == beta


def test_stats_clear_and_the_library_refuses():
    """The ABI through ctypes: each refusal with its status code and message, before anything is allocated; read and clear."""
    dev = D.Dagger("sac", 3, 2, 2, 2, [-1, -1], [1, 1], beta=1.0)
    lib, vp = dev.lib, ctypes.c_void_p
    err = lambda: lib.hrg_last_error().decode()   # noqa: E731
    f = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype).cuda()   # noqa: E731
    rows = f(3, ACT, dtype=torch.float64)
    dev.step(f(3, 2), f(3, 2), f(3, ACT, dtype=torch.float64), rows)   # kept_out None
    assert dev.stats()["steps"] == 3 and dev.stats()["steps"] == 0   # read and clear
    dev.beta = 1.5
    with pytest.raises(ValueError, match="beta = 1.5 outside"):
        dev.step(f(3, 2), f(3, 2), f(3, ACT, dtype=torch.float64), rows)
    dev.beta = 1.0
    with pytest.raises(ValueError, match="view: expected a contiguous torch.float32 tensor"):
        dev.step(f(3, 3), f(3, 2), f(3, ACT, dtype=torch.float64), rows)
    ptr = lambda x: vp(x.data_ptr())   # noqa: E731
    tb = dev.table
    args = lambda beta, obs=tb.observations: (ptr(f(3, 2)), ptr(f(3, 2)), ptr(f(3, ACT, dtype=torch.float64)), beta, None if obs is None else ptr(obs), ptr(tb.actions), ptr(rows), None, None)  # noqa: E731
    for beta in (-0.5, 1.5, float("nan")):
        assert lib.hrg_dagger_step(dev.h, *args(beta)) == CONST["HRG_ERR_INVALID"] and "dagger: beta" in err()
    assert lib.hrg_dagger_step(dev.h, *args(0.5, None)) == CONST["HRG_ERR_INVALID"] and "dagger: null table" in err()
    assert dev.sizes()["n_calls"] == 1   # no refused call counted as a step

    def create(**kw):
        d, out = DaggerDesc(), vp()
        d.kind, d.n_envs, d.obs_dim, d.act_dim, d.capacity_steps = CONST["HRG_BC_SAC"], 3, 2, 2, 2
        for j in range(ACT):
            d.act_low[j], d.act_high[j] = -1.0, 1.0
        for k, v in kw.items():
            if k in ("act_low", "act_high"):
                getattr(d, k)[v[0]] = v[1]
            else:
                setattr(d, k, v)
        rc = lib.hrg_dagger_create(ctypes.byref(d), 0, ctypes.byref(out))
        return rc, out

    for kw, code, what in ((dict(obs_dim=0), "HRG_ERR_UNSUPPORTED", "dagger: obs_dim = 0"), (dict(obs_dim=65), "HRG_ERR_UNSUPPORTED", "dagger: obs_dim = 65"),
                           (dict(act_dim=0), "HRG_ERR_UNSUPPORTED", "dagger: act_dim = 0"), (dict(act_dim=8), "HRG_ERR_UNSUPPORTED", "dagger: act_dim = 8"),
                           (dict(capacity_steps=0), "HRG_ERR_INVALID", "dagger: capacity_steps = 0"), (dict(act_high=(1, -1.0)), "HRG_ERR_INVALID", "dagger: action bound 1"),
                           (dict(act_high=(0, float("inf"))), "HRG_ERR_INVALID", "dagger: action bound 0"), (dict(kind=2), "HRG_ERR_INVALID", "dagger: kind = 2"),
                           (dict(n_envs=0), "HRG_ERR_INVALID", "dagger: n_envs = 0"), (dict(pinned_rows=-1), "HRG_ERR_INVALID", "dagger: pinned_rows = -1")):
        rc, out = create(**kw)
        assert rc == CONST[code] and what in err() and not out.value, kw
    rc, out = create(act_high=(5, -3.0))   # a bound behind act_dim is not read
    assert rc == CONST["HRG_OK"] and out.value
    lib.hrg_dagger_destroy(out)
    dev.close()


# ---- on the env
def _reach(n, horizon, seed=5, shield="SSM", norm=False, **kw):
    rng = np.random.RandomState(0)
    obs_norm = dict(mean=rng.uniform(-0.5, 0.5, 18), std=rng.uniform(0.5, 2.0, 18)) if norm else None
    return hrg.HipVecEnv(n, env_kwargs=dict(horizon=horizon, seed=seed, shield_type=shield), clips=_clips(), obs_norm=obs_norm,
                         expert=dict(id="ReachHuman", signal_to_noise_ratio=1.0), **kw)


def test_beta_zero_is_collect_steps():
    n, steps = 8, 16
    envs = [_reach(n, 12, norm=True) for _ in range(2)]
    for env in envs:
        env.attach_replay(n * 32)
        env.attach_sac(batch_size=32)
    a, b = envs
    dg = a.attach_dagger(n * 32, beta=0.0)
    assert a.collect_dagger(steps) is dg
    b.collect_steps(lambda o: b.sac.act(o, deterministic=True), steps)
    ea, eb = a.replay.export(), b.replay.export()
    assert sorted(ea) == sorted(eb) and ea["pos"] == steps and ea["dones"].any()   # (episodes ended and started again on the way)
    for k in ea:
        np.testing.assert_array_equal(ea[k], eb[k], err_msg=k)
    assert torch.equal(a._backend.batch.obs, b._backend.batch.obs)
    table = dg.table
    assert table.n_rows == steps * n and (table.obs_dim, table.act_dim, table.kind) == (18, 7, "sac")
    np.testing.assert_array_equal(table.observations[:steps * n].cpu().numpy().reshape(steps, n, 18), ea["observations"][:steps])   # what the learner was shown
    st = dg.stats()
    assert (st["steps"], st["expert_steps"], st["expert_fraction"]) == (steps * n, 0, 0.0) and st["imitation_error"] > 0
    lab = table.actions[:steps * n].cpu().numpy()
    assert np.abs(lab).max() <= 1.0 and np.abs(lab).max() > 0
    with pytest.raises(RuntimeError, match="step_async after collect_dagger"):
        a.step_async(np.zeros((n, 7)))
    for env in envs:
        env.close()


def test_beta_one_is_the_expert_driving():
    n, steps = 4, 10
    env, twin = _reach(n, 6), _reach(n, 6)
    env.attach_replay(n * 16)
    env.attach_sac(batch_size=32)
    dg = env.attach_dagger(n * 16, beta=1.0)
    env.collect_dagger(steps)
    twin.reset()
    rewards, dones = [], []
    for _ in range(steps):
        _, r, d, _ = twin.step(twin.expert_actions())
        rewards.append(np.array(r, np.float32))
        dones.append(np.array(d))
    assert np.array(dones).any()
    assert torch.equal(env._backend.batch.obs, twin._backend.batch.obs)
    st = dg.stats()
    assert (st["steps"], st["expert_steps"], st["expert_fraction"]) == (steps * n, steps * n, 1.0)
    ex = env.replay.export()
    np.testing.assert_array_equal(ex["rewards"][:steps], np.array(rewards))
    np.testing.assert_array_equal(ex["actions"][:steps].reshape(steps * n, 7), dg.table.actions[:steps * n].cpu().numpy())   # the buffer keeps the label
    env.close()
    twin.close()


def test_cartesian_labels_behind_the_ik_front_end():
    n, steps, ENV = 5, 3, "ReachHumanCart"
    env = hrg.HipVecEnv(n, env_id=ENV, env_kwargs=dict(horizon=6, seed=3), clips=task_clips(ENV, 2, min_frames=200, max_frames=300), expert=dict(id=ENV),
                        ik_position_delta=dict(action_limit=0.1))
    env.attach_rollout(32)
    learner = env.attach_ppo(batch_size=32, net_arch=[64, 64])
    dg = env.attach_dagger(n * 8, beta=0.5)
    assert (dg.table.kind, dg.table.act_dim, dg.table.obs_dim, learner.act_dim) == ("ppo", 4, env.rollout.obs_dim, 4)
    low, high = np.asarray(env.action_space.low, np.float64), np.asarray(env.action_space.high, np.float64)
    b, path = env._backend.batch, env._device_path
    # the loop's own steps, one by one, so that each step's expert buffer and executed rows can be read
    sent, experts = [], []
    launch = path._step
    path._step = lambda rows: (experts.append(b._expert_act.cpu().numpy().copy()), sent.append(rows.cpu().numpy().copy()), launch(rows))[-1]
    env.collect_dagger(steps)
    path._step = launch
    assert len(sent) == steps and env.rollout.pos == 0   # no slot of the rollout buffer is written
    for t in range(steps):
        lab = dg.table.actions[t * n:(t + 1) * n].cpu().numpy()
        np.testing.assert_array_equal(lab, np.clip(experts[t][:, :4], low, high).astype(np.float32))
        assert not sent[t][:, 4:].any() and np.abs(sent[t][:, :3]).max() <= high[0]
    assert np.abs(np.array(experts)[:, :, :3]).max() > 0
    st = dg.stats()
    assert st["steps"] == steps * n and 0 < st["expert_steps"] < steps * n
    assert torch.equal(env.rollout.observation(), env.rollout.view(b.obs))   # the buffer's current rows followed the envs
    env.collect_rollout(learner.policy, learner.value)   # the on-policy loop goes on, from a reset
    assert env.rollout.full
    env.close()


def test_bc_on_the_growing_table(oracle_lib):
    n, batch = 8, 32
    env = _reach(n, 12)
    env.attach_replay(n * 8)
    env.attach_sac(batch_size=32)
    dg = env.attach_dagger(n * 4)   # four step slots
    bc = env.attach_bc(dg.table, batch_size=batch)
    assert bc.table is dg.table and dg.table.n_rows == 0
    with pytest.raises(ValueError, match=r"behaviour cloning: the table is empty \(n_rows = 0\)"):
        bc.step()
    with pytest.raises(ValueError, match="the table is empty"):
        bc.train(2)
    assert bc.n_updates == 0
    for t in range(1, 7):
        env.collect_dagger(1)
        rows = min(t, 4) * n
        assert dg.table.n_rows == rows == dg.sizes()["n_rows"]
        newest = (t - 1) % 4
        seen = []
        for _ in range(2):
            count = bc.n_updates
            bc.step()
            idx = bc.export()["indices"]
            np.testing.assert_array_equal(idx, bc_ref.draw(oracle_lib.hrgo_test_u01, int(bc.desc.seed), count, batch, rows))   # drawn from the rows written so far
            seen.append(idx)
        seen = np.concatenate(seen)
        assert seen.min() >= 0 and seen.max() < rows
        assert ((seen >= newest * n) & (seen < (newest + 1) * n)).any(), t   # rows of the newest slot are drawn
    assert np.isfinite(bc.diagnostics()["loss"]) and bool(torch.isfinite(env.sac.p.params).all())
    env.close()


def test_it_learns():
    """A random-init SAC actor, three iterations of (collect with beta = 0.5, behaviour cloning on the aggregate): the on-policy imitation error -- measured by
    collect_dagger(H, beta = 0), the learner driving every step -- falls.  A sign condition; the measured ratio is recorded in DESIGN.md §7."""
    n, H = 64, 20
    env = _reach(n, H, shield="OFF")
    env.attach_replay(n * H * 8)
    env.attach_sac(batch_size=128)
    dg = env.attach_dagger(n * H * 8, beta=0.0)
    bc = env.attach_bc(dg.table, batch_size=128, learning_rate=1e-3)

    def on_policy_error():
        dg.beta = 0.0
        dg.stats()   # (clear)
        env.collect_dagger(H)
        st = dg.stats()
        assert st["steps"] == n * H and st["expert_steps"] == 0
        return st["imitation_error"]

    before = on_policy_error()
    for i in range(3):
        dg.beta = 0.5
        env.collect_dagger(H)
        st = dg.stats()
        assert 0.35 < st["expert_fraction"] < 0.65   # 1280 draws at 0.5: +-0.15 is ten standard deviations
        bc.train(300)
    after = on_policy_error()
    print(f"[dagger] on-policy imitation error {before:.4e} -> {after:.4e} (ratio {after / before:.3f}); bc loss {bc.diagnostics()['loss']:.4e}")
    assert np.isfinite(after) and after < before
    env.close()


def test_lifecycle_on_the_device():
    n = 4
    env = _reach(n, 6)
    env.attach_replay(n * 8)
    env.attach_sac(batch_size=32)
    first = env.attach_dagger(n * 4, beta=1.0, seed=7)
    assert env.dagger is first and first.desc.seed == 7 and first.desc.capacity_steps == 4 and first.desc.env_id0 == 0
    second = env.attach_dagger(n * 2)
    assert env.dagger is second and not first.h.value and second.desc.seed == 5 and second.beta == 0.5   # replaced: the first handle is destroyed; the env's seed
    env.collect_dagger(3)
    assert second.table.n_rows == 2 * n and second.n_calls == 3 and second.sizes()["slot"] == 1
    bc = env.attach_bc(second.table, batch_size=32)
    env.seed(9)
    third = env.dagger
    assert third is not second and not second.h.value and third.table is not second.table
    assert third.table.n_rows == 0 and third.n_calls == 0 and third.sizes() == dict(n_calls=0, slot=0, n_rows=0, bytes=third.sizes()["bytes"])
    assert not third.table.observations.any() and third.stats()["steps"] == 0 and third.desc.seed == 9
    assert bc.table is third.table   # the cloning goes on, on the new table
    env.collect_dagger(1)
    assert third.table.n_rows == n
    env.close()
    assert env.dagger is None and not third.h.value
