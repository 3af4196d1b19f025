"""The PPO minibatch step on the device (csrc/hrgym_ppo.h) against tests/ppo_ref.py, the restatement from torch's own parts on the CPU.  -m gpu.

The yardstick is the float32 noise floor: `ref64` is the restatement in float64, `ref32` the same code in float32, and for a tensor X
err(X) = max|X_dev - X_ref64| / max|X_ref64|, floor(X) the same for ref32.  One step: err <= 8 floor + 2^-22; twenty steps: err <= 8 floor20 + 2^-20.
Nothing is held against the code under test.  Every err and floor is printed before it is asserted (run with -s).

Shapes: minibatches of 32 (one tile) and 96 (three tiles, not a power of two) and one of 4096 (128 tiles), observations of 1, 6 and 64 values, actions of 1, 4
and 7, a shared trunk of depth 1 and 3 and separate trunks of depth 2.  The inputs keep every row at least 0.02 away from the kinks of the two clamps
(ppo_ref.make_rows; ppo_ref.assert_conditions holds that, on 1e-3, against ref64 and ref32 before the device is looked at): a reference and the device may
otherwise fall on different sides of one."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import ppo_ref as R
from helpers import _dev, _err
import human_robot_gym_amd as hrg
from human_robot_gym_amd._lib import HrgError
from human_robot_gym_amd.ppo import DIAG_KEYS, PpoLearner
from human_robot_gym_amd.rollout import RolloutBuffer, RolloutBufferSamples, build_rollout_desc

pytestmark = pytest.mark.gpu

LR, ENT_COEF, VF_COEF, CLIP = 3e-4, 0.01, 0.5, 0.2
ARCHS = ((1, False), (3, False), (2, True))   # depth, separate
# normalize_advantage, clip_range_vf, max_grad_norm: 100 lies above every case's gradient norm and 0.01 below (test_gradient_norm_on_both_sides_of_max_grad_norm)
VARIANTS = ((True, None, 0.5), (False, 0.2, 100.0), (True, 0.2, 0.01), (False, None, 0.5))
SHAPES = list(itertools.product((1, 6, 64), (1, 4, 7), ARCHS, (32, 96))) + [(18, 7, (2, False), 4096)]   # obs_dim, act_dim, (depth, separate), batch
GROUP_PREFIXES = ("mlp_extractor.shared_net.", "mlp_extractor.policy_net.", "mlp_extractor.value_net.", "action_net.", "value_net.", "log_std")
SCALARS = ("policy_gradient_loss", "value_loss", "entropy_loss", "approx_kl")


def _net_arch(depth, separate):
    return [dict(pi=[64] * depth, vf=[64] * depth)] if separate else [64] * depth


def _samples(batch):
    return RolloutBufferSamples(**{k: _dev(batch[k]) for k in RolloutBufferSamples._fields})


def _cfg(depth, separate, variant=0, lr=LR):
    norm, clip_vf, max_norm = VARIANTS[variant]
    return R.Cfg(depth, separate, lr, CLIP, clip_vf, norm, ENT_COEF, VF_COEF, max_norm)


def _learner(K, A, cfg, B, params=None, seed=1, **kw):
    lr = PpoLearner(K, A, net_arch=_net_arch(cfg.depth, cfg.separate), learning_rate=cfg.lr, batch_size=B, clip_range=cfg.clip_range, clip_range_vf=cfg.clip_range_vf,
                    normalize_advantage=cfg.normalize_advantage, ent_coef=cfg.ent_coef, vf_coef=cfg.vf_coef, max_grad_norm=cfg.max_grad_norm, seed=seed, **kw)
    if params is not None:
        lr.load_state_dict(params)
    return lr


def _flat(named, prefix):
    """The entries of `named` under `prefix` as one vector, in the layout's order; None when there is none."""
    parts = [np.asarray(v.detach().cpu(), np.float64).reshape(-1) for k, v in named.items() if k.startswith(prefix)]
    return np.concatenate(parts) if parts else None


@functools.lru_cache(maxsize=None)
def _one_step(K, A, arch, B):
    """One step of ref64, ref32 and the device from the same case; computed once, shared by the tests and left unchanged."""
    depth, separate = arch
    cfg = _cfg(depth, separate, SHAPES.index((K, A, arch, B)) % len(VARIANTS))
    p, batch = R.make_case(K, A, depth, separate, B, seed=100 * K + 10 * A + depth + (5 if separate else 0))
    s64, s32 = R.RefState(p, torch.float64), R.RefState(p, torch.float32)
    o64, o32 = s64.step(batch, cfg), s32.step(batch, cfg)
    for o in (o64, o32):
        R.assert_conditions(o, batch, cfg)
    lr = _learner(K, A, cfg, B, p)
    before = {k: v.clone().cpu() for k, v in lr.state_dict().items()}
    lr.step(_samples(batch))
    ex = lr.export()
    after = {k: v.clone().cpu() for k, v in lr.state_dict().items()}
    named = lambda flat: {k: torch.as_tensor(flat)[off:off + int(np.prod(shape))].reshape(shape).cpu().clone() for k, (off, shape) in lr.p.layout.items()}   # noqa: E731
    out = dict(cfg=cfg, p=p, o64=o64, o32=o32, ex=ex, before=before, after=after, grad=named(ex["grad"]), m=named(lr.p.adam_m), v=named(lr.p.adam_v), diag=lr.diagnostics())
    lr.close()
    return out


@pytest.mark.parametrize("K, A, arch, B", SHAPES)
def test_one_step_intermediates_and_gradients(K, A, arch, B):
    c = _one_step(K, A, arch, B)
    o64, o32, ex = c["o64"], c["o32"], c["ex"]
    rows = {k: (ex[k], o64[k], o32[k]) for k in ("values", "log_prob", "ratio")}
    for k in SCALARS:
        rows[k] = (ex["diag"][k], o64["losses"][k], o32["losses"][k])
    for prefix in GROUP_PREFIXES:
        if _flat(o64["grad"], prefix) is not None:
            rows["grad " + prefix] = (_flat(c["grad"], prefix), _flat(o64["grad"], prefix), _flat(o32["grad"], prefix))
    assert len(rows) == 7 + (5 if arch[1] else 4)
    rows["grad_norm"] = (ex["diag"]["grad_norm"], o64["grad_norm"], o32["grad_norm"])
    bad = []
    for k, (dev, r64, r32) in rows.items():
        err, floor = _err(dev, r64, r32)
        print(f"[ppo] K {K} A {A} arch {arch} B {B} {k}: err {err:.2e} floor {floor:.2e} ratio {err / max(floor, 1e-300):.2f}")
        if not err <= 8 * floor + 2.0 ** -22:
            bad.append(k)
    assert not bad, bad
    assert ex["diag"]["clip_fraction"] == o64["losses"]["clip_fraction"] == o32["losses"]["clip_fraction"]   # exact: a count over B
    for k in ("loss", "std"):   # what diagnostics() reports is the step's own
        assert c["diag"][k] == pytest.approx(o64["losses"][k], rel=1e-4, abs=1e-6), k
    assert c["diag"]["n_updates"] == 1 and c["diag"]["clip_range"] == CLIP and c["diag"]["learning_rate"] == LR
    assert ("clip_range_vf" in c["diag"]) == (c["cfg"].clip_range_vf is not None)


def test_gradient_norm_on_both_sides_of_max_grad_norm():
    below = above = 0
    for K, A, arch, B in SHAPES[:8]:   # two of every variant
        c = _one_step(K, A, arch, B)
        n64, n32, mx = c["o64"]["grad_norm"], c["o32"]["grad_norm"], c["cfg"].max_grad_norm
        print(f"[ppo] K {K} A {A} arch {arch} B {B}: gradient norm {n64:.4f}, max_grad_norm {mx}")
        below += int(n64 < mx and n32 < mx)
        above += int(n64 > mx and n32 > mx)
        if mx == 100.0:
            assert n64 < mx and n32 < mx
        if mx == 0.01:
            assert n64 > mx and n32 > mx
    assert below >= 2 and above >= 2


@pytest.mark.parametrize("K, A, arch, B", SHAPES)
def test_one_step_adam_from_the_device_gradient(K, A, arch, B):
    """Parameters and moments after the step, from the device's own gradient: clip_grad_norm_ and torch.optim.Adam(eps=1e-5) in float64 on that gradient.  The
    device computes the update in double and rounds once: 2^-23 of the value, plus 2^-20 of the learning rate for the update's own rounding."""
    c = _one_step(K, A, arch, B)
    cfg = c["cfg"]
    want, m, v, coef = R.adam_from_gradient({k: x.double() for k, x in c["before"].items()}, {k: g.double() for k, g in c["grad"].items()}, cfg)
    norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in c["grad"].values()))
    assert c["ex"]["diag"]["grad_norm"] == pytest.approx(norm, rel=2.0 ** -22)
    assert (coef < 1.0) == (norm > cfg.max_grad_norm)
    for k in want:
        p0, p1 = c["before"][k].double(), c["after"][k].double()
        upd = (p0 - want[k]).abs() / cfg.lr
        bound = 2.0 ** -23 * want[k].abs() + 2.0 ** -20 * cfg.lr * torch.clamp(upd, min=1.0)
        assert bool(((p1 - want[k]).abs() <= bound).all()), k
        assert bool(((c["m"][k].double() - m[k]).abs() <= 2.0 ** -23 * m[k].abs() + 1e-30).all()), k
        assert bool(((c["v"][k].double() - v[k]).abs() <= 2.0 ** -23 * v[k].abs() + 1e-30).all()), k


def test_the_library_refuses_what_the_host_refuses():
    """hrg_ppo_create checks the descriptor again: every field the Python side refuses, set behind its back."""
    import ctypes
    from human_robot_gym_amd._lib import load_library
    from human_robot_gym_amd.ppo import build_ppo_desc
    lib = load_library()
    for field, value, match in (("use_sde", 1, "use_sde"), ("target_kl_set", 1, "target_kl"), ("policy", 1, "MlpPolicy"), ("hidden", 128, "hidden width 64"),
                                ("depth", 0, "depth = 0"), ("depth", 4, "depth = 4"), ("separate", 2, "separate"), ("obs_dim", 0, "obs_dim = 0"), ("obs_dim", 65, "obs_dim = 65"),
                                ("act_dim", 0, "act_dim = 0"), ("act_dim", 8, "act_dim = 8"), ("batch_size", 48, "batch_size = 48"), ("batch_size", 8192, "batch_size = 8192"),
                                ("rollout_size", 96, "no short last minibatch"), ("ent_coef", -1.0, "ent_coef"), ("max_grad_norm", 0.0, "max_grad_norm")):
        d = build_ppo_desc(6, 7, net_arch=[64, 64], batch_size=64, rollout_size=128)
        setattr(d, field, value)
        h = ctypes.c_void_p()
        assert lib.hrg_ppo_create(ctypes.byref(d), 0, ctypes.byref(h)) != 0 and not h.value, field
        assert match in lib.hrg_last_error().decode(), (field, lib.hrg_last_error().decode())
    lr = PpoLearner(6, 7, net_arch=[64, 64], batch_size=64)
    bad = RolloutBufferSamples(*(torch.zeros(64, n).cuda() if n else torch.zeros(64).cuda() for n in (6, 7, 0, 0, 0, 0)))
    with pytest.raises(ValueError, match="observations"):
        lr.step(bad._replace(observations=torch.zeros(64, 5).cuda()))
    lr.clip_range = 0.0
    with pytest.raises(HrgError, match="clip_range"):
        lr.step(bad)
    lr.clip_range, lr.clip_range_vf = 0.2, -0.5
    with pytest.raises(ValueError, match="clip_range_vf"):
        lr.step(bad)
    assert lr.n_updates == 0
    lr.close()


def _fill_rollout(K, A, cfg, p, n, n_steps, seed, margin):
    """A real RolloutBuffer filled with synthetic rows whose ratios and values under `p` sit `margin` away from the kinks; returns (buffer, its export)."""
    from human_robot_gym_amd._cstruct import CONST
    g = torch.Generator().manual_seed(seed)
    rb = RolloutBuffer(build_rollout_desc(n, n_steps, list(range(K)), act_dim=A, gamma=0.99, gae_lambda=0.9), seed=seed)
    rows = (torch.rand(n_steps + 1, n, 64, generator=g, dtype=torch.float64) * 2.0 - 1.0).float()
    rb.observe(rows[0].cuda())
    for t in range(n_steps):
        r = R.make_rows(p, rows[t][:, :K].double(), cfg.depth, cfg.separate, g, clip_range=cfg.clip_range, clip_range_vf=0.2, margin=margin)
        done = (torch.rand(n, generator=g) < 0.15).to(torch.uint8)
        rb.add_step(_dev(r["actions"]), _dev(r["old_values"]), _dev(r["old_log_prob"]), None, rows[t + 1].cuda(), None, _dev(torch.randn(n, generator=g)), done.cuda(),
                    torch.zeros(n, CONST["HRG_INFO_DIM"], dtype=torch.int32).cuda())
    rb.compute_returns_and_advantage(_dev(torch.randn(n, generator=g)))
    return rb, rb.export()


def _ref_batch(ex, idx):
    return dict(observations=ex["observations"][idx], actions=ex["actions"][idx], old_values=ex["values"][idx], old_log_prob=ex["log_probs"][idx],
                advantages=ex["advantages"][idx], returns=ex["returns"][idx])


@pytest.mark.parametrize("K, A, arch, B, variant", [(6, 4, (3, False), 96, 2), (18, 7, (2, True), 64, 1)])
def test_twenty_steps(K, A, arch, B, variant):
    """Twenty steps through a real RolloutBuffer, the minibatches from explicit indices, the same for the device and the references.  The learning rate (3e-5) and
    the rows' distance from the kinks (0.08) are this test's: twenty steps move no row of ref64 or ref32 to within 1e-3 of a kink, which is asserted at every step."""
    depth, separate = arch
    cfg = _cfg(depth, separate, variant, lr=3e-5)
    p = R.make_params(K, A, depth, separate, seed=7)
    rb, ex = _fill_rollout(K, A, cfg, p, n=24, n_steps=8, seed=3, margin=0.08)
    assert ex["computed"] and (ex["advantages"] > 0).any() and (ex["advantages"] < 0).any()
    s64, s32 = R.RefState(p, torch.float64), R.RefState(p, torch.float32)
    lr = _learner(K, A, cfg, B, p, rollout_size=24 * 8)
    rng = np.random.RandomState(0)
    for step in range(20):
        idx = rng.permutation(24 * 8)[:B]
        batch, = rb.get(indices=torch.from_numpy(idx).cuda())
        lr.step(batch)
        for s in (s64, s32):
            o = s.step(_ref_batch(ex, idx), cfg)
            R.assert_conditions(o, _ref_batch(ex, idx), cfg)
    bad = []
    for k, v in lr.state_dict().items():
        err, floor = _err(v.cpu(), s64.p[k].detach(), s32.p[k].detach())
        print(f"[ppo] twenty steps K {K} A {A} arch {arch} B {B} {k}: err {err:.2e} floor20 {floor:.2e}")
        if not err <= 8 * floor + 2.0 ** -20:
            bad.append(k)
    assert not bad, bad
    assert lr.n_updates == 20
    lr.close()
    rb.close()


@pytest.mark.parametrize("K, A, arch", [(6, 4, (3, False)), (64, 7, (1, True)), (1, 1, (2, True)), (18, 7, (2, False))])
def test_policy_and_value(K, A, arch):
    depth, separate = arch
    cfg = _cfg(depth, separate)
    p = R.make_params(K, A, depth, separate, seed=5)
    ref = R.RefState(p, torch.float64)
    a, b = _learner(K, A, cfg, 32, p, seed=4), _learner(K, A, cfg, 32, p, seed=4)
    g = torch.Generator().manual_seed(0)
    own = 0
    for n in (1, 63, 64, 65, 321):
        obs = torch.randn(n, K, generator=g, dtype=torch.float64).float()
        eps = (0.3 * torch.randn(n, A, generator=g, dtype=torch.float64)).float()
        det, sto = a.policy(obs.cuda(), deterministic=True), a.policy(obs.cuda(), eps=eps.cuda())
        val = a.value(obs.cuda())
        assert tuple(det[0].shape) == (n, A) and tuple(det[1].shape) == tuple(det[2].shape) == tuple(val.shape) == (n,) and all(x.dtype == torch.float32 for x in det)
        for what, got, want in (("deterministic", det, ref.forward(obs, cfg)), ("eps", sto, ref.forward(obs, cfg, eps))):
            for name, x, y in zip(("actions", "values", "log_probs"), got, want):
                d = float((x.cpu().double() - y).abs().max())
                print(f"[ppo] policy K {K} A {A} arch {arch} n {n} {what} {name}: max difference {d:.2e}")
                assert d <= 2.0 ** -20
        assert float((val.cpu().double() - ref.forward(obs, cfg)[1]).abs().max()) <= 2.0 ** -20
        assert torch.equal(val, det[1])
        x1, x2, y1 = a.policy(obs.cuda()), a.policy(obs.cuda()), b.policy(obs.cuda())   # the call counter keys the draws
        own += 2
        assert not torch.equal(x1[0], x2[0]) and all(torch.equal(u, w) for u, w in zip(x1, y1))
        assert torch.equal(x1[1], val) and bool(torch.isfinite(x1[0]).all()) and bool(torch.isfinite(x1[2]).all())
        # the log_prob handed out is that of the float32 action under the reference's distribution
        mu, _, _ = ref.forward(obs, cfg)
        lp = R.log_prob_closed_form(mu, ref.p["log_std"].detach(), x1[0].cpu().double())
        assert float((x1[2].cpu().double() - lp).abs().max()) <= 2.0 ** -18
        b.policy(obs.cuda())
    assert a._sizes()[4] == b._sizes()[4] == own   # explicit noise, deterministic calls and value() do not move the counter
    a.close()
    b.close()


def test_own_draws_are_standard_normal():
    K, A = 6, 7
    cfg = _cfg(2, False)
    lr = _learner(K, A, cfg, 32, R.make_params(K, A, 2, False, seed=5), seed=9)
    obs = torch.zeros(4096, K).cuda()
    act, _, _ = lr.policy(obs)
    mu, _, _ = lr.policy(obs, deterministic=True)
    z = ((act - mu) / lr.state_dict()["log_std"].exp()).cpu().double()
    print(f"[ppo] own draws: mean {float(z.mean()):.4f} std {float(z.std()):.4f}")
    assert abs(float(z.mean())) < 0.03 and abs(float(z.std()) - 1.0) < 0.03   # 28672 draws: three standard errors are 0.018 and 0.013
    assert abs(float(np.corrcoef(z[:, 0].numpy(), z[:, 1].numpy())[0, 1])) < 0.06
    lr.close()


def test_determinism():
    K, A, n, n_steps = 18, 4, 16, 8
    cfg = _cfg(2, False)
    state = []
    for seed in (3, 3, 4):
        rb, _ = _fill_rollout(K, A, cfg, R.make_params(K, A, 2, False, seed=1), n, n_steps, seed=11, margin=0.02)
        lr = PpoLearner(K, A, net_arch=[64, 64], batch_size=32, n_epochs=3, ortho_init=False, seed=seed, rollout_size=n * n_steps)
        lr.train(rb)
        assert lr.n_updates == 3 * n * n_steps // 32
        state.append({k: v.cpu().numpy().tobytes() for k, v in lr.state_dict().items()})
        lr.close()
        rb.close()
    assert state[0] == state[1]
    assert all(state[0][k] != state[2][k] for k in state[0])


def test_it_learns_a_one_step_problem():
    """A constant observation, r = -|a - a*|^2, every step terminal: the advantage is r - V and the return r.  The device and ref32 each sample from their own
    parameters with shared noise and run the same 150 rounds of one sample and four minibatch steps; both bring |mu - a*| below a fifth of where it started,
    and the device ends within twice ref32's distance plus 0.01.  (The learning rate, 3e-3, a* = (0.6, -0.5) and the sizes -- one tile, depth 1, two actions,
    log_std -0.5 -- are this test's: the smallest problem with the whole step in it; ref32 alone meets the criterion on the CPU.)"""
    K, A, B, rounds, epochs = 3, 2, 32, 150, 4
    cfg = R.Cfg(1, False, 3e-3, 0.2, None, True, 0.0, 0.5, 0.5)
    target = torch.tensor([0.6, -0.5], dtype=torch.float64)
    p = R.make_params(K, A, 1, False, seed=11)
    ref = R.RefState(p, torch.float32)
    dev = _learner(K, A, cfg, B, p)
    obs1 = torch.tensor([[0.3, -0.2, 0.1]], dtype=torch.float64)
    obs = obs1.repeat(B, 1)
    obs_d = _dev(obs)
    dist = lambda a: float((a.double().reshape(-1) - target).norm())   # noqa: E731
    start = dist(ref.forward(obs1, cfg)[0])
    g = torch.Generator().manual_seed(2)
    eps = torch.randn(rounds, B, A, generator=g, dtype=torch.float64).float()
    eps_d = eps.cuda()
    target_d = target.float().cuda()
    for s in range(rounds):
        act, val, lp = dev.policy(obs_d, eps=eps_d[s])
        rew = -((act - target_d) ** 2).sum(-1)
        batch = RolloutBufferSamples(obs_d, act, val, lp, rew - val, rew)
        act_r, val_r, lp_r = ref.forward(obs, cfg, eps[s])
        rew_r = -((act_r.double() - target) ** 2).sum(-1).float()
        batch_r = dict(observations=obs, actions=act_r, old_values=val_r, old_log_prob=lp_r, advantages=rew_r - val_r, returns=rew_r)
        for _ in range(epochs):
            dev.step(batch)
            ref.step(batch_r, cfg, outputs=False)
    end_ref, end_dev = dist(ref.forward(obs1, cfg)[0]), dist(dev.policy(_dev(obs1), deterministic=True)[0].cpu())
    print(f"[ppo] one-step problem: distance {start:.4f} -> ref32 {end_ref:.4f}, device {end_dev:.4f}")
    assert start > 0.2
    assert end_ref < start / 5 and end_dev < start / 5
    assert end_dev <= 2 * end_ref + 0.01
    dev.close()


def test_through_the_env():
    kw = dict(env_kwargs=dict(horizon=4, seed=11, shield_type="OFF"), clips=hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300))
    env = hrg.HipVecEnv(64, **kw)
    with pytest.raises(NotImplementedError, match="attach_rollout"):
        env.attach_ppo(batch_size=64)
    rb = env.attach_rollout(8, gamma=0.99, gae_lambda=0.9)
    with pytest.raises(NotImplementedError, match="no short last minibatch"):
        env.attach_ppo(batch_size=96)
    assert env.ppo is None
    ppo = env.attach_ppo(batch_size=64, n_epochs=3, learning_rate=LR, net_arch=[64, 64], log_std_init=-2.7, ortho_init=False, full_std=True, use_expln=False, squash_output=True)
    assert env.ppo is ppo and (ppo.obs_dim, ppo.act_dim, ppo.batch_size) == (rb.obs_dim, rb.act_dim, 64) and ppo.desc.seed == 11 and ppo.desc.rollout_size == 512
    before = {k: v.clone() for k, v in ppo.state_dict().items()}
    assert env.collect_rollout(ppo.policy, ppo.value) is rb and rb.full
    ppo.train(rb)
    after = ppo.state_dict()
    assert all(bool(torch.isfinite(v).all()) for v in after.values())
    moved = lambda prefix: max(float((after[k] - before[k]).abs().max()) for k in after if k.startswith(prefix))   # noqa: E731
    assert moved("mlp_extractor.shared_net.") > 0 and moved("action_net.") > 0 and moved("value_net.") > 0 and moved("log_std") > 0
    diag = ppo.diagnostics()
    assert set(diag) == set(DIAG_KEYS) | {"clip_range", "learning_rate", "n_updates"} and all(math.isfinite(v) for v in diag.values())
    assert diag["n_updates"] == ppo.n_updates == 3 * 512 // 64
    assert 0.0 <= diag["clip_fraction"] <= 1.0 and diag["approx_kl"] >= 0.0 and diag["std"] == pytest.approx(float(after["log_std"].exp().mean()), rel=1e-2)
    # load_state_dict(state_dict()) is the identity
    flat = ppo.p.params.clone()
    ppo.load_state_dict({k: v.clone() for k, v in after.items()})
    assert torch.equal(ppo.p.params, flat)
    # weights from torch modules: the deterministic forward pass is the modules'
    K, A = ppo.obs_dim, ppo.act_dim
    torch.manual_seed(5)
    shared = torch.nn.Sequential(torch.nn.Linear(K, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh())
    action_net, value_net = torch.nn.Linear(64, A), torch.nn.Linear(64, 1)
    state = {k: v.clone() for k, v in after.items()}
    for prefix, mod in (("mlp_extractor.shared_net", shared), ("action_net", action_net), ("value_net", value_net)):
        for k, v in mod.state_dict().items():
            state[f"{prefix}.{k}"] = v
    assert set(state) == set(after)
    ppo.load_state_dict(state)
    obs = rb.observation()
    with torch.no_grad():
        h = shared(obs.cpu().double().float())
        want_a, want_v = action_net(h), value_net(h).squeeze(-1)
    got_a, got_v, _ = ppo.policy(obs, deterministic=True)
    assert float((got_a.cpu() - want_a).abs().max()) <= 2.0 ** -20 and float((got_v.cpu() - want_v).abs().max()) <= 2.0 ** -20
    assert float((ppo.value(obs).cpu() - want_v).abs().max()) <= 2.0 ** -20
    # separate trunks through the same env
    sep = env.attach_ppo(batch_size=128, n_epochs=1, net_arch=[dict(pi=[64], vf=[64])])
    assert env.ppo is sep and sep.separate and sep.depth == 1
    b0 = {k: v.clone() for k, v in sep.state_dict().items()}
    env.collect_rollout(sep.policy, sep.value)
    sep.train(rb)
    assert sep.n_updates == 4 and all(bool(torch.isfinite(v).all()) and not torch.equal(v, b0[k]) for k, v in sep.state_dict().items())
    env.close()
