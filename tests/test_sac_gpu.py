"""The SAC gradient step on the device (csrc/hrgym_sac.h) against tests/sac_ref.py, the torch-autograd restatement on the CPU.  -m gpu.

The yardstick is the float32 noise floor: `ref64` is the restatement in float64, `ref32` the same code in float32, and for a tensor X
err(X) = max|X_dev - X_ref64| / max|X_ref64|, floor(X) the same for ref32.  One step: err <= 8 floor + 2^-22; twenty steps: err <= 8 floor20 + 2^-20.
Nothing is held against the code under test.  Every err and floor is printed before it is asserted (run with -s).

Shapes: batches of 32 (one tile) and 160 (five tiles, not a power of two), observations of 1, 6 and 64 values, actions of 1, 4 and 7, depths 1 and 3.  The
inputs meet every branch (sac_ref.make_case; sac_ref.assert_branches holds that against ref64 before the device is looked at).

Measured on one MI355X (this file, -s): the figures are in DESIGN.md D22."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import sac_ref as R
from helpers import _dev, _err
import human_robot_gym_amd as hrg
from human_robot_gym_amd._lib import HrgError
from human_robot_gym_amd.replay import ReplayBufferSamples
from human_robot_gym_amd.sac import SacLearner, Q_COLUMNS

pytestmark = pytest.mark.gpu

LR, GAMMA, TAU = 5e-4, 0.99, 0.005
SHAPES = list(itertools.product((1, 6, 64), (1, 4, 7), (1, 3), (32, 160)))   # obs_dim, act_dim, depth, batch
GROUPS = (("actor", "actor."), ("qf0", "critic.qf0."), ("qf1", "critic.qf1."), ("log_ent_coef", "log_ent_coef"))


def _samples(batch):
    return ReplayBufferSamples(**{k: _dev(batch[k]) for k in ReplayBufferSamples._fields})


def _learner(K, A, depth, B, params=None, ent_coef="auto_0.2", seed=1, **kw):
    lr = SacLearner(K, A, net_arch=[64] * depth, learning_rate=LR, gamma=GAMMA, tau=TAU, ent_coef=ent_coef, batch_size=B, seed=seed, **kw)
    if params is not None:
        lr.load_state_dict(params)
    return lr


def _cfg(A, depth, auto=True, ent_coef=0.2, interval=1, lr=LR):
    return R.Cfg(depth, lr, GAMMA, TAU, auto, ent_coef, -float(A), interval)


def _flat(named, prefix, layout):
    """The entries of `named` under `prefix` as one vector, in the order of the device's parameter vector."""
    return np.concatenate([np.asarray(named[k].detach().cpu(), np.float64).reshape(-1) for k in layout if k.startswith(prefix)])


@functools.lru_cache(maxsize=None)
def _one_step(K, A, depth, B):
    """One step of ref64, ref32 and the device from the same case; computed once, shared by the tests and left unchanged."""
    p, batch, e1, e2 = R.make_case(K, A, depth, B, seed=100 * K + 10 * A + depth)
    s64, s32 = R.RefState(p, torch.float64), R.RefState(p, torch.float32)
    o64, o32 = s64.step(batch, e1, e2, _cfg(A, depth)), s32.step(batch, e1, e2, _cfg(A, depth))
    R.assert_branches(p, batch, e1, e2, o64, depth)
    lr = _learner(K, A, depth, B, p)
    before = {k: v.clone().cpu() for k, v in lr.state_dict().items()}
    lr.step(_samples(batch), _dev(e1), _dev(e2))
    ex = lr.export()
    after = {k: v.clone().cpu() for k, v in lr.state_dict().items()}
    groups = {g: lr.p.group(torch.from_numpy(ex["grad"]), g).numpy().copy() for g, _ in GROUPS}
    flat_grad = {k: ex["grad"][off:off + int(np.prod(shape))].reshape(shape) for k, (off, shape) in lr.p.layout.items()}
    diag, layout = lr.diagnostics(), list(lr.p.layout)
    lr.close()
    return dict(layout=layout, p=p, o64=o64, o32=o32, s64=s64, s32=s32, ex=ex, before=before, after=after, groups=groups, grad=flat_grad, diag=diag)


@pytest.mark.parametrize("K, A, depth, B", SHAPES)
def test_one_step_intermediates_and_gradients(K, A, depth, B):
    c = _one_step(K, A, depth, B)
    o64, o32, ex = c["o64"], c["o32"], c["ex"]
    rows = {k: (ex[k], o64[k], o32[k]) for k in ("y", "logp", "logp_next")}
    for i, k in enumerate(Q_COLUMNS):
        rows[k] = (ex["q"][i], o64["q"][k], o32["q"][k])
    for g, prefix in GROUPS:
        rows["grad " + g] = (c["groups"][g], _flat(o64["grad"], prefix, c["layout"]), _flat(o32["grad"], prefix, c["layout"]))
    bad = []
    for k, (dev, r64, r32) in rows.items():
        err, floor = _err(dev, r64, r32)
        print(f"[sac] K {K} A {A} depth {depth} B {B} {k}: err {err:.2e} floor {floor:.2e} ratio {err / max(floor, 1e-300):.2f}")
        if not err <= 8 * floor + 2.0 ** -22:
            bad.append(k)
    assert not bad, bad
    for k in ("actor_loss", "critic_loss", "ent_coef_loss", "ent_coef"):   # what diagnostics() reports is the step's own
        assert c["diag"][k] == pytest.approx(o64["losses"][k], rel=1e-4, abs=1e-6), k
    assert c["diag"]["n_updates"] == 1


@pytest.mark.parametrize("K, A, depth, B", SHAPES)
def test_one_step_adam_and_polyak_from_the_device_gradient(K, A, depth, B):
    c = _one_step(K, A, depth, B)
    zero_seen = 0
    for k, g in c["grad"].items():
        p0, p1 = c["before"][k].double(), c["after"][k].double()
        want = p0.clone()
        upd = R.adam_update(want, torch.from_numpy(g.astype(np.float64)), torch.zeros_like(want), torch.zeros_like(want), 1, LR)
        bound = 2.0 ** -23 * want.abs() + 2.0 ** -20 * LR * torch.clamp(upd.abs(), min=1.0)
        assert bool(((p1 - want).abs() <= bound).all()), k
        zero = c["o64"]["grad"][k] == 0   # exactly zero in ref64 (dead units, log_std rows clamped in every row): exactly zero on the device, the value unchanged
        zero_seen += int(zero.sum())
        assert bool((torch.from_numpy(g)[zero] == 0).all()) and bool((p1[zero] == p0[zero]).all()), k
        if k.startswith("critic."):
            tk = "critic_target." + k[len("critic."):]
            t_want = (1.0 - TAU) * c["before"][tk].double() + TAU * p1
            assert bool(((c["after"][tk].double() - t_want).abs() <= 2.0 ** -22 * t_want.abs()).all()), tk
    assert zero_seen > 0
    if A >= 3:   # the two log_std rows that clamp in every row of the batch
        assert bool((c["o64"]["grad"]["actor.log_std.weight"][:2] == 0).all())


@pytest.mark.parametrize("K, A, depth, B, interval", [(6, 4, 3, 160, 1), (64, 7, 1, 32, 2)])
def test_twenty_steps(K, A, depth, B, interval):
    p, _, _, _ = R.make_case(K, A, depth, B, seed=7)
    s64, s32 = R.RefState(p, torch.float64), R.RefState(p, torch.float32)
    lr = _learner(K, A, depth, B, p, target_update_interval=interval)
    cfg = _cfg(A, depth, interval=interval)
    tname = f"critic_target.qf1.{2 * depth}.weight"
    for step in range(20):
        _, batch, e1, e2 = R.make_case(K, A, depth, B, seed=1000 + step)
        t0 = lr.state_dict()[tname].clone()
        lr.step(_samples(batch), _dev(e1), _dev(e2))
        s64.step(batch, e1, e2, cfg)
        s32.step(batch, e1, e2, cfg)
        assert (not torch.equal(t0, lr.state_dict()[tname])) == (step % interval == 0), f"targets at step {step}"
    bad = []
    for k, v in lr.state_dict().items():
        err, floor = _err(v.cpu(), s64.p[k], s32.p[k])
        print(f"[sac] twenty steps K {K} A {A} depth {depth} B {B} {k}: err {err:.2e} floor20 {floor:.2e}")
        if not err <= 8 * floor + 2.0 ** -20:
            bad.append(k)
    assert not bad, bad
    assert lr.n_updates == 20
    lr.close()


def test_fixed_and_initial_entropy_coefficient():
    K, A, depth, B = 6, 4, 3, 32
    p, batch, e1, e2 = R.make_case(K, A, depth, B, seed=3)
    fixed = _learner(K, A, depth, B, p, ent_coef=0.1)
    before = fixed.state_dict()["log_ent_coef"].clone()
    fixed.step(_samples(batch), _dev(e1), _dev(e2))
    ex, o64 = fixed.export(), R.RefState(p, torch.float64).step(batch, e1, e2, _cfg(A, depth, auto=False, ent_coef=0.1))
    o32 = R.RefState(p, torch.float32).step(batch, e1, e2, _cfg(A, depth, auto=False, ent_coef=0.1))
    assert torch.equal(fixed.state_dict()["log_ent_coef"], before) and ex["grad"][-1] == 0 and fixed.diagnostics()["ent_coef"] == pytest.approx(0.1, rel=1e-6)
    for k in ("y", "logp"):   # the fixed coefficient is the one in y and in the actor's loss
        err, floor = _err(ex[k], o64[k], o32[k])
        print(f"[sac] ent_coef 0.1 {k}: err {err:.2e} floor {floor:.2e}")
        assert err <= 8 * floor + 2.0 ** -22
    err, floor = _err(fixed.p.group(torch.from_numpy(ex["grad"]), "actor").numpy(), _flat(o64["grad"], "actor.", fixed.p.layout), _flat(o32["grad"], "actor.", fixed.p.layout))
    print(f"[sac] ent_coef 0.1 grad actor: err {err:.2e} floor {floor:.2e}")
    assert err <= 8 * floor + 2.0 ** -22
    fixed.close()
    auto = SacLearner(K, A, net_arch=[64] * depth, ent_coef="auto_0.2", batch_size=B, seed=1)   # its own initial parameters
    assert float(auto.state_dict()["log_ent_coef"]) == pytest.approx(math.log(0.2), rel=1e-7)
    p2 = {k: v.cpu().clone() for k, v in auto.state_dict().items()}
    auto.step(_samples(batch), _dev(e1), _dev(e2))
    ex = auto.export()
    cfg = _cfg(A, depth)
    o64, o32 = R.RefState(p2, torch.float64).step(batch, e1, e2, cfg), R.RefState(p2, torch.float32).step(batch, e1, e2, cfg)
    want = -(o64["logp"] + cfg.target_entropy).mean()   # target_entropy "auto": -act_dim
    assert float(o64["grad"]["log_ent_coef"]) == pytest.approx(float(want), rel=1e-12)
    err, floor = _err(ex["grad"][-1:], o64["grad"]["log_ent_coef"], o32["grad"]["log_ent_coef"])
    print(f"[sac] auto_0.2 coefficient gradient: err {err:.2e} floor {floor:.2e}")
    assert err <= 8 * floor + 2.0 ** -22
    assert auto.diagnostics()["ent_coef"] == pytest.approx(0.2, rel=1e-6) and not torch.equal(auto.state_dict()["log_ent_coef"].cpu(), p2["log_ent_coef"])
    auto.close()


@pytest.mark.parametrize("K, A, depth", [(6, 4, 3), (64, 7, 1), (1, 1, 3)])
def test_act(K, A, depth):
    p = R.make_params(K, A, depth, seed=5)   # (plain initial weights: the case builder's log_std head, scaled to reach both clamps, magnifies float32 rounding past 2^-20)
    ref = R.RefState(p, torch.float64)
    a, b = _learner(K, A, depth, 32, p, seed=4), _learner(K, A, depth, 32, p, seed=4)
    g = torch.Generator().manual_seed(0)
    for n in (1, 63, 64, 65, 321):
        obs = torch.randn(n, K, generator=g, dtype=torch.float64).float()
        eps = (0.3 * torch.randn(n, A, generator=g, dtype=torch.float64)).float()
        det, sto = a.act(obs.cuda(), deterministic=True).cpu(), a.act(obs.cuda(), eps=eps.cuda()).cpu()
        assert tuple(det.shape) == (n, A) and det.dtype == torch.float32
        for got, want in ((det, ref.act(obs)), (sto, ref.act(obs, eps))):
            d = float((got.double() - want).abs().max())
            print(f"[sac] act K {K} A {A} depth {depth} n {n}: max difference {d:.2e}")
            assert d <= 2.0 ** -20
        x1, x2, y1 = a.act(obs.cuda()).cpu(), a.act(obs.cuda()).cpu(), b.act(obs.cuda()).cpu()   # the call counter keys the draws
        for x in (det, x1, x2):
            assert bool((x.abs() < 1).all()) and bool(torch.isfinite(x).all())
        assert not torch.equal(x1, x2) and torch.equal(x1, y1)
        b.act(obs.cuda())
    assert a._sizes()[4] == b._sizes()[4] == 10   # explicit noise and deterministic calls do not move the counter
    a.close()
    b.close()


def _fill(buf, n, steps, seed):
    from human_robot_gym_amd._cstruct import CONST
    rng = np.random.RandomState(seed)
    buf.observe(_dev(rng.uniform(-1, 1, (n, 64))))
    for _ in range(steps):
        buf.add_step(_dev(rng.uniform(-1, 1, (n, buf.act_dim))), _dev(rng.uniform(-1, 1, (n, 64))), _dev(rng.uniform(-1, 1, (n, 64))), _dev(rng.normal(size=n)),
                     torch.from_numpy((rng.uniform(size=n) < 0.2).astype(np.uint8)).cuda(), torch.zeros(n, CONST["HRG_INFO_DIM"], dtype=torch.int32).cuda())


def test_determinism():
    from human_robot_gym_amd.replay import ReplayBuffer, build_replay_desc
    K, A, n = 18, 4, 10
    state = []
    for seed, buffer_seed in ((3, 11), (3, 11), (4, 11)):
        buf = ReplayBuffer(build_replay_desc(n, n * 6, list(range(K)), act_dim=A, seed=buffer_seed))
        _fill(buf, n, 6, seed=0)
        lr = SacLearner(K, A, ent_coef="auto_0.2", batch_size=64, seed=seed)
        lr.train(buf, 10)
        assert lr.n_updates == 10
        state.append({k: v.cpu().numpy().tobytes() for k, v in lr.state_dict().items()})
        lr.close()
        buf.close()
    assert state[0] == state[1]
    assert all(state[0][k] != state[2][k] for k in state[0] if k != "log_ent_coef")   # (the coefficient starts from the same value in all three)


def test_it_learns_a_one_step_problem():
    """r = -|a - a*|^2, every transition terminal: Q(a) = r, and the actor's mean goes to a*.  The device and ref32 run the same 1500 steps on the same batches
    and noise; both bring |tanh(mu) - a*| below a fifth of where it started, and the device ends within twice ref32's distance plus 0.01.  (The learning rate,
    2e-3, a* = (0.6, -0.5) and the sizes -- one tile, depth 1, two actions -- are this test's: the smallest problem with the whole step in it.)"""
    K, A, depth, B, steps, lr_ = 3, 2, 1, 32, 1500, 2e-3
    target = torch.tensor([0.6, -0.5], dtype=torch.float64)
    p = R.make_params(K, A, depth, seed=11)
    ref = R.RefState(p, torch.float32)
    dev = _learner(K, A, depth, B, p)
    dev.learning_rate = lr_
    cfg = _cfg(A, depth, lr=lr_)
    obs1 = torch.tensor([[0.3, -0.2, 0.1]], dtype=torch.float64)
    obs = obs1.repeat(B, 1)
    dist = lambda a: float((a.double().reshape(-1) - target).norm())   # noqa: E731
    start = dist(ref.act(obs1))
    g = torch.Generator().manual_seed(2)
    acts = torch.rand(steps, B, A, generator=g, dtype=torch.float64) * 2.0 - 1.0
    eps = torch.randn(steps, 2, B, A, generator=g, dtype=torch.float64)
    acts_d, eps_d, obs_d = _dev(acts), _dev(eps), _dev(obs)
    rew = -((acts - target) ** 2).sum(-1, keepdim=True)
    rew_d, ones_d = _dev(rew), torch.ones(B, 1, dtype=torch.float32).cuda()
    for s in range(steps):
        dev.step(ReplayBufferSamples(obs_d, acts_d[s], obs_d, ones_d, rew_d[s]), eps_d[s, 0], eps_d[s, 1])
        ref.step(dict(observations=obs, actions=acts[s], next_observations=obs, dones=torch.ones(B, 1), rewards=rew[s]), eps[s, 0], eps[s, 1], cfg)
    end_ref, end_dev = dist(ref.act(obs1)), dist(dev.act(_dev(obs1), deterministic=True).cpu())
    print(f"[sac] one-step problem: distance {start:.4f} -> ref32 {end_ref:.4f}, device {end_dev:.4f}")
    assert start > 0.2
    assert end_ref < start / 5 and end_dev < start / 5
    assert end_dev <= 2 * end_ref + 0.01
    dev.close()


def test_through_the_env():
    rng = np.random.RandomState(0)
    kw = dict(env_kwargs=dict(horizon=4, seed=11, shield_type="OFF"), clips=hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300),
              obs_norm=dict(mean=rng.uniform(-0.5, 0.5, 64), std=rng.uniform(0.5, 2.0, 64), allow_different_observation_shapes=True))
    env = hrg.HipVecEnv(64, **kw)
    with pytest.raises(NotImplementedError, match="attach_replay"):
        env.attach_sac(batch_size=32)
    rb = env.attach_replay(6400)
    sac = env.attach_sac(batch_size=32, learning_rate=LR, ent_coef="auto_0.2")
    assert env.sac is sac and (sac.obs_dim, sac.act_dim, sac.batch_size) == (rb.obs_dim, rb.act_dim, 32) and sac.desc.seed == 11
    with pytest.raises(HrgError, match="empty"):
        sac.train(rb, 1)
    before = {k: v.clone() for k, v in sac.state_dict().items()}
    assert env.collect_steps(sac.act, 5) is rb and rb.size() == 5
    sac.train(rb, 4)
    after = sac.state_dict()
    assert all(bool(torch.isfinite(v).all()) for v in after.values())
    moved = lambda prefix: max(float((after[k] - before[k]).abs().max()) for k in after if k.startswith(prefix))   # noqa: E731
    assert moved("actor.") > 0 and moved("critic.qf0.") > 0 and moved("critic.qf1.") > 0 and moved("log_ent_coef") > 0
    assert 0 < moved("critic_target.") < min(moved("critic.qf0."), moved("critic.qf1."))
    diag = sac.diagnostics()
    assert set(diag) == {"ent_coef", "actor_loss", "critic_loss", "ent_coef_loss", "n_updates"} and all(math.isfinite(v) for v in diag.values()) and diag["n_updates"] == 4
    # load_state_dict(state_dict()) is the identity
    flat = sac.p.params.clone(), sac.p.target.clone()
    sac.load_state_dict({k: v.clone() for k, v in after.items()})
    assert torch.equal(sac.p.params, flat[0]) and torch.equal(sac.p.target, flat[1])
    # weights from torch modules: the actor's forward pass is the modules'
    K, A = sac.obs_dim, sac.act_dim
    torch.manual_seed(5)
    mlp = lambda i, o: torch.nn.Sequential(torch.nn.Linear(i, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.ReLU(),  # noqa: E731
                                           *([torch.nn.Linear(64, o)] if o else []))
    latent, qf0, qf1, mu, log_std = mlp(K, 0), mlp(K + A, 1), mlp(K + A, 1), torch.nn.Linear(64, A), torch.nn.Linear(64, A)
    state = {k: v.clone() for k, v in after.items()}
    for prefix, mod in (("actor.latent_pi", latent), ("actor.mu", mu), ("actor.log_std", log_std), ("critic.qf0", qf0), ("critic.qf1", qf1),
                        ("critic_target.qf0", qf0), ("critic_target.qf1", qf1)):
        for k, v in mod.state_dict().items():
            state[f"{prefix}.{k}"] = v
    assert set(state) == set(after)
    sac.load_state_dict(state)
    obs = rb.observation()
    with torch.no_grad():
        want = torch.tanh(mu(latent(obs.cpu().double().float())))
    assert float((sac.act(obs, deterministic=True).cpu() - want).abs().max()) <= 2.0 ** -20
    env.close()
