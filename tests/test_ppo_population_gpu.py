"""The PPO population on the device (csrc/hrgym_ppo.h): P learners in the same four launches.  -m gpu.

The specification is exact: member p of a population equals, bit for bit, a lone PpoLearner with member p's seed on the same rows -- every sum has an order that
does not depend on the launch, a member's advantage statistics, clip coefficient and diagnostics come from its own sums, and every draw is keyed (seed, forward
call count, row within the member's group, stream, component).  So every comparison with a lone learner here is torch.equal / np.array_equal; there is no
tolerance.  The one comparison that has one is with the independent float64 restatement (tests/ppo_ref.py), on tests/test_ppo_gpu.py's bound."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import ppo_ref as R
from helpers import _dev, _err
import human_robot_gym_amd as hrg
from human_robot_gym_amd._cstruct import CONST
from human_robot_gym_amd._lib import _ptr, load_library
from human_robot_gym_amd.ppo import PpoLearner, PpoPopulation, build_ppo_desc
from human_robot_gym_amd.rollout import RolloutBuffer, RolloutBufferSamples, build_rollout_desc

pytestmark = pytest.mark.gpu

LR, ENT_COEF, VF_COEF, CLIP = 3e-4, 0.01, 0.5, 0.2
TENSORS = ("params", "adam_m", "adam_v")
EXPORT_KEYS = ("values", "log_prob", "ratio", "grad", "diag")
SHAPES = ((6, 4, [64], 32), (18, 7, [dict(pi=[64, 64], vf=[64, 64])], 64), (5, 1, [64, 64, 64], 96))   # K, A, net_arch, B: one tile; two networks, two tiles; three tiles
POPULATIONS = ((1, (4,)), (2, (8, 8 + 2**40)), (3, (5, 9, 2)))   # P, seeds (not consecutive; one beyond 32 bits)


def _arch(net_arch):
    separate = isinstance(net_arch[0], dict)
    return (len(net_arch[0]["pi"]) if separate else len(net_arch)), separate


@functools.lru_cache(maxsize=None)
def _case(K, A, depth, separate, B, seed):
    """(parameters, minibatch on the device) of ppo_ref.make_case; computed once, shared and left unchanged."""
    p, batch = R.make_case(K, A, depth, separate, B, seed=seed)
    return p, RolloutBufferSamples(**{k: _dev(batch[k]) for k in RolloutBufferSamples._fields}), batch


def _stack(batches):
    return RolloutBufferSamples(*(torch.cat(xs).contiguous() for xs in zip(*batches)))


def _assert_member(pop, p, lone, what):
    for name in TENSORS:
        assert torch.equal(getattr(pop.p, name)[p], getattr(lone.p, name)), (what, p, name)
    assert pop._sizes()[3:5] == lone._sizes()[3:5], (what, p, "counters")


def _assert_exports(pop, p, lone, what):
    got, want = pop.export(member=p), lone.export()
    for k in EXPORT_KEYS[:4]:
        assert np.array_equal(got[k], want[k]), (what, p, k)
    assert got["diag"] == want["diag"], (what, p, "diag")


@pytest.mark.parametrize("normalize, clip_range_vf", [(True, None), (False, 0.2), (True, 0.2), (False, None)])
@pytest.mark.parametrize("K, A, net_arch, B", SHAPES)
@pytest.mark.parametrize("P, seeds", POPULATIONS)
def test_a_member_is_the_lone_learner_of_its_seed(P, seeds, K, A, net_arch, B, normalize, clip_range_vf):
    depth, separate = _arch(net_arch)
    kw = dict(net_arch=net_arch, learning_rate=LR, batch_size=B, clip_range=CLIP, clip_range_vf=clip_range_vf, normalize_advantage=normalize, ent_coef=ENT_COEF,
              vf_coef=VF_COEF, log_std_init=-0.5)
    pop = PpoPopulation(K, A, P, seeds, **kw)
    lones = [PpoLearner(K, A, seed=s, **kw) for s in seeds]
    assert tuple(pop.p.params.shape) == (P, lones[0].p.n_params) and pop.seeds == list(seeds)
    for step in range(3):   # a different minibatch for every member and step
        batches = [_case(K, A, depth, separate, B, 100 * step + 7 * p + K)[1] for p in range(P)]
        pop.step(_stack(batches))
        for p, lone in enumerate(lones):
            lone.step(batches[p])
            _assert_exports(pop, p, lone, f"step {step}")
    for p, lone in enumerate(lones):
        _assert_member(pop, p, lone, "after three steps")
    diag = pop.diagnostics()
    assert len(diag) == P and all(d == lone.diagnostics() for d, lone in zip(diag, lones)) and diag[0]["n_updates"] == 3
    if P > 1:   # members of different seeds and minibatches are different learners (a population that shares parameters or scratch fails here)
        assert not torch.equal(pop.p.params[0], pop.p.params[1]) and not np.array_equal(pop.export(0)["log_prob"], pop.export(1)["log_prob"])
        assert pop.export(0)["diag"]["grad_norm"] != pop.export(1)["diag"]["grad_norm"]
    with pytest.raises(ValueError, match="observations"):   # [P * B] rows, no more and no fewer
        pop.step(batches[0] if P > 1 else _stack(batches + batches))
    with pytest.raises(NotImplementedError, match="member"):
        pop.state_dict()
    pop.close()
    for lone in lones:
        lone.close()


GROUP_PREFIXES = ("mlp_extractor.shared_net.", "mlp_extractor.policy_net.", "mlp_extractor.value_net.", "action_net.", "value_net.", "log_std")
SCALARS = ("policy_gradient_loss", "value_loss", "entropy_loss", "approx_kl")


def _flat(named, prefix):
    parts = [np.asarray(v.detach().cpu(), np.float64).reshape(-1) for k, v in named.items() if k.startswith(prefix)]
    return np.concatenate(parts) if parts else None


@pytest.mark.parametrize("K, A, net_arch, B, normalize, clip_range_vf", [(18, 7, [dict(pi=[64, 64], vf=[64, 64])], 64, True, 0.2), (6, 4, [64], 32, False, None)])
def test_one_member_against_the_independent_restatement(K, A, net_arch, B, normalize, clip_range_vf):
    """Member 1 of two after one step against tests/ppo_ref.py in float64, on tests/test_ppo_gpu.py::test_one_step_intermediates_and_gradients' yardstick:
    err(X) = max|X_dev - X_ref64| / max|X_ref64| <= 8 floor(X) + 2^-22, floor the same for the float32 run of the reference.  Member 0 holds other parameters
    and steps on another minibatch."""
    depth, separate = _arch(net_arch)
    cfg = R.Cfg(depth, separate, LR, CLIP, clip_range_vf, normalize, ENT_COEF, VF_COEF, 0.5)
    cases = [_case(K, A, depth, separate, B, 31), _case(K, A, depth, separate, B, 100 * K + 10 * A + depth)]
    pop = PpoPopulation(K, A, 2, (3, 11), net_arch=net_arch, learning_rate=LR, batch_size=B, clip_range=CLIP, clip_range_vf=clip_range_vf, normalize_advantage=normalize,
                        ent_coef=ENT_COEF, vf_coef=VF_COEF)
    for m, (p, _, _) in enumerate(cases):
        for name, (off, shape) in pop.p.layout.items():
            pop.p.params[m, off:off + int(np.prod(shape))] = _dev(p[name]).reshape(-1)
    p, _, batch = cases[1]
    o64, o32 = R.RefState(p, torch.float64).step(batch, cfg), R.RefState(p, torch.float32).step(batch, cfg)
    for o in (o64, o32):
        R.assert_conditions(o, batch, cfg)
    pop.step(_stack([c[1] for c in cases]))
    ex = pop.export(member=1)
    grad = {k: torch.as_tensor(ex["grad"])[off:off + int(np.prod(shape))] for k, (off, shape) in pop.p.layout.items()}
    rows = {k: (ex[k], o64[k], o32[k]) for k in ("values", "log_prob", "ratio")}
    for k in SCALARS:
        rows[k] = (ex["diag"][k], o64["losses"][k], o32["losses"][k])
    for prefix in GROUP_PREFIXES:
        if _flat(o64["grad"], prefix) is not None:
            rows["grad " + prefix] = (_flat(grad, prefix), _flat(o64["grad"], prefix), _flat(o32["grad"], prefix))
    assert len(rows) == 7 + (5 if separate else 4)
    rows["grad_norm"] = (ex["diag"]["grad_norm"], o64["grad_norm"], o32["grad_norm"])
    bad = []
    for k, (dev, r64, r32) in rows.items():
        err, floor = _err(dev, r64, r32)
        print(f"[ppo population] K {K} A {A} B {B} member 1 {k}: err {err:.2e} floor {floor:.2e}")
        if not err <= 8 * floor + 2.0 ** -22:
            bad.append(k)
    assert not bad, bad
    assert ex["diag"]["clip_fraction"] == o64["losses"]["clip_fraction"] == o32["losses"]["clip_fraction"]   # exact: a count over B
    assert not np.array_equal(pop.export(member=0)["values"], ex["values"])
    pop.close()


def test_forward_keeps_to_the_group():
    P, seeds, K, A, m = 3, (5, 9, 2), 6, 4, 40   # 40 rows: a full tile and one of 8 rows per group
    kw = dict(net_arch=[dict(pi=[64], vf=[64])], batch_size=32, log_std_init=-0.5)
    pop = PpoPopulation(K, A, P, seeds, **kw)
    lones = [PpoLearner(K, A, seed=s, **kw) for s in seeds]
    rng = np.random.RandomState(3)
    obs = torch.from_numpy(rng.uniform(-1, 1, (P * m, K)).astype(np.float32)).cuda()
    group = lambda x, p: x[p * m:(p + 1) * m]   # noqa: E731
    for call in range(2):   # (seed_p, forward call count, row within the group, STREAM_PPO_ACT, j)
        got = pop.policy(obs)
        assert tuple(got[0].shape) == (P * m, A) and tuple(got[1].shape) == tuple(got[2].shape) == (P * m,)
        for p, lone in enumerate(lones):
            want = lone.policy(group(obs, p).contiguous())
            for name, x, y in zip(("actions", "values", "log_probs"), got, want):
                assert torch.equal(group(x, p), y), ("own draws", call, p, name)
    assert not torch.equal(group(got[0], 0), group(got[0], 1))
    values = pop.value(obs)
    det = pop.policy(obs, deterministic=True)
    for p, lone in enumerate(lones):
        assert torch.equal(group(values, p), lone.value(group(obs, p).contiguous())), ("value", p)
        assert all(torch.equal(group(x, p), y) for x, y in zip(det, lone.policy(group(obs, p).contiguous(), deterministic=True))), ("deterministic", p)
    assert torch.equal(values, det[1]) and pop._sizes()[4] == 2 == lones[0]._sizes()[4]   # value() and deterministic calls do not move the counter
    # another group's observations do not reach a group's outputs
    other = obs.clone()
    other[m:2 * m] = 7.0
    moved, moved_values = pop.policy(other, deterministic=True), pop.value(other)
    for p in (0, 2):
        assert all(torch.equal(group(x, p), group(y, p)) for x, y in zip(moved, det)) and torch.equal(group(moved_values, p), group(values, p)), p
    assert not torch.equal(group(moved[0], 1), group(det[0], 1))
    # the ragged tile of a group ends at the group: a lone forward on group 0's rows into poisoned arrays leaves the next group's rows alone, and the
    # population's last group leaves what lies behind the arrays' rows alone
    poison = 12345.0
    fresh = lambda: (torch.full((P * m + 32, A), poison, device="cuda"), torch.full((P * m + 32,), poison, device="cuda"), torch.full((P * m + 32,), poison, device="cuda"))   # noqa: E731
    lone = lones[0]
    a, v, lp = fresh()
    lone._check(lone.lib, lone.lib.hrg_ppo_forward(lone.h, _ptr(lone.p.params), _ptr(obs), m, None, 1, _ptr(a), _ptr(v), _ptr(lp), lone._stream()))
    assert torch.equal(a[:m], det[0][:m]) and torch.equal(v[:m], det[1][:m]) and torch.equal(lp[:m], det[2][:m])
    assert bool((a[m:] == poison).all()) and bool((v[m:] == poison).all()) and bool((lp[m:] == poison).all())
    a, v, lp = fresh()
    pop._check(pop.lib, pop.lib.hrg_ppo_population_forward(pop.h, _ptr(pop.p.params), _ptr(obs), m, None, 1, _ptr(a), _ptr(v), _ptr(lp), pop._stream()))
    assert torch.equal(a[:P * m], det[0]) and torch.equal(v[:P * m], det[1]) and torch.equal(lp[:P * m], det[2])
    assert bool((a[P * m:] == poison).all()) and bool((v[P * m:] == poison).all()) and bool((lp[P * m:] == poison).all())
    a, v, lp = fresh()   # the values alone
    pop._check(pop.lib, pop.lib.hrg_ppo_population_forward(pop.h, _ptr(pop.p.params), _ptr(obs), m, None, 1, None, _ptr(v), None, pop._stream()))
    assert torch.equal(v[:P * m], values) and bool((v[P * m:] == poison).all()) and bool((a == poison).all()) and bool((lp == poison).all())
    with pytest.raises(ValueError, match="groups of the same size"):
        pop.policy(obs[:P * m - 1].contiguous())
    pop.close()
    for lone in lones:
        lone.close()


def _rows(n, T, K, A, seed):
    """Random rows for a buffer of `n` envs and `T` steps, on the host: what observe / add_step / compute_returns_and_advantage take, by env."""
    g = torch.Generator().manual_seed(seed)
    return dict(obs=(torch.rand(T + 1, n, 64, generator=g) * 2.0 - 1.0), actions=torch.randn(T, n, A, generator=g), values=torch.randn(T, n, generator=g),
                log_probs=torch.randn(T, n, generator=g), reward=torch.randn(T, n, generator=g), done=(torch.rand(T, n, generator=g) < 0.15).to(torch.uint8),
                last=torch.randn(n, generator=g))


def _filled(rows, envs, T, K, A, seed):
    """A computed RolloutBuffer of the envs `envs` (a slice) of `rows`."""
    n = envs.stop - envs.start
    rb = RolloutBuffer(build_rollout_desc(n, T, list(range(K)), act_dim=A, gamma=0.99, gae_lambda=0.9), seed=seed)
    cut = lambda x: x[:, envs].contiguous().cuda()   # noqa: E731
    obs, actions, values, log_probs, reward, done = (cut(rows[k]) for k in ("obs", "actions", "values", "log_probs", "reward", "done"))
    rb.observe(obs[0])
    for t in range(T):
        rb.add_step(actions[t], values[t], log_probs[t], None, obs[t + 1], None, reward[t], done[t], torch.zeros(n, CONST["HRG_INFO_DIM"], dtype=torch.int32).cuda())
    rb.compute_returns_and_advantage(rows["last"][envs].contiguous().cuda())
    return rb


def test_grouped_minibatches_are_the_lone_buffers():
    G, m, T, K, A, B, seeds = 3, 4, 8, 18, 4, 16, (21, 4, 2**63 + 5)
    rows = _rows(G * m, T, K, A, seed=0)
    big = _filled(rows, slice(0, G * m), T, K, A, seed=99)
    lones = [_filled(rows, slice(m * g, m * (g + 1)), T, K, A, seed=s) for g, s in enumerate(seeds)]
    stored = big.export()
    for epoch in range(2):   # the generators go on from epoch to epoch, as the lone buffers' do
        got = list(big.get_groups(G, B, seeds))
        table = big.last_indices
        assert tuple(table.shape) == (G, m * T) and table.dtype == torch.int64 and len(got) == m * T // B
        want = [list(lone.get(B)) for lone in lones]
        for g, lone in enumerate(lones):
            assert torch.equal(table[g], lone.last_indices + g * m * T), (epoch, g)   # the lone buffer's permutation, moved into the group's range
            assert sorted(table[g].tolist()) == list(range(g * m * T, (g + 1) * m * T)), (epoch, g)   # its range, exactly once
            for k, batch in enumerate(got):
                assert tuple(batch.observations.shape) == (G * B, K) and tuple(batch.returns.shape) == (G * B,)
                for name, x, y in zip(RolloutBufferSamples._fields, batch, want[g][k]):
                    assert torch.equal(x[g * B:(g + 1) * B], y), (epoch, g, k, name)
        idx = torch.cat([table[:, k * B:(k + 1) * B].reshape(-1) for k in range(len(got))]).cpu().numpy()
        for name, key in (("observations", "observations"), ("actions", "actions"), ("old_values", "values"), ("old_log_prob", "log_probs"), ("advantages", "advantages"),
                          ("returns", "returns")):
            assert np.array_equal(torch.cat([getattr(b, name) for b in got]).cpu().numpy(), stored[key][idx]), name
    again = list(big.get_groups(G, B, seeds[::-1]))   # another seeds list reseeds the generators
    fresh = RolloutBuffer(build_rollout_desc(m, T, list(range(K)), act_dim=A), seed=seeds[2])
    assert len(again) == 2 and torch.equal(big.last_indices[0], torch.randperm(m * T, device="cuda", generator=fresh.generator))
    with pytest.raises(NotImplementedError, match="n_envs = 12 is not divisible by n_groups = 5"):
        big.get_groups(5, B, range(5))
    with pytest.raises(NotImplementedError, match=r"batch_size = 24 does not divide m \* n_steps = 32"):
        big.get_groups(G, 24, seeds)
    with pytest.raises(ValueError, match="2 seeds for 3 groups"):
        big.get_groups(G, B, (1, 2))
    for b in [big, fresh] + lones:
        b.close()


PER_STEP = ("observations", "actions", "rewards", "values", "log_probs", "episode_starts", "advantages", "returns")   # [n * n_steps, ...], i = env * n_steps + step
PER_ENV = ("cur_obs", "flags", "run_return", "run_length", "stats")                                                  # [n, ...]


def test_population_end_to_end_equals_lone_runs_on_the_groups():
    P, m, T, seeds = 2, 8, 8, (3, 7)
    kw = dict(batch_size=32, n_epochs=2, learning_rate=LR, net_arch=[64, 64], log_std_init=-1.0, ortho_init=False)
    clips = hrg.synthetic_clips(3, seed=0, min_frames=200, max_frames=300)
    ek = dict(horizon=10, seed=5)
    env = hrg.HipVecEnv(P * m, env_id="ReachHuman", env_kwargs=ek, clips=clips)
    with pytest.raises(NotImplementedError, match="attach_ppo_population: call attach_rollout"):
        env.attach_ppo_population(P, seeds=seeds, **kw)
    env.attach_rollout(T, gamma=0.99, gae_lambda=0.9)
    with pytest.raises(NotImplementedError, match="attach_ppo_population: n_envs = 16 is not divisible by n_groups = 3"):
        env.attach_ppo_population(3, **kw)
    with pytest.raises(NotImplementedError, match=r"attach_ppo_population: batch_size = 96 does not divide m \* n_steps = 64"):
        env.attach_ppo_population(P, seeds=seeds, **dict(kw, batch_size=96))
    assert env.ppo_population is None
    pop = env.attach_ppo_population(P, seeds=seeds, **kw)
    assert env.ppo_population is pop and pop.seeds == list(seeds) and pop.desc.rollout_size == m * T
    assert env.attach_ppo_population(P, **kw).seeds == [5, 6]   # the default: the env's seed + p; the earlier population is closed
    assert not pop.h.value
    pop = env.attach_ppo_population(P, seeds=seeds, **kw)
    for _ in range(2):
        assert env.collect_rollout(pop.policy, pop.value) is env.rollout
        pop.train(env.rollout)
    assert pop.n_updates == 2 * 2 * (m * T // 32)
    got, got_stats = env.rollout.export(), env.rollout.episode_stats(clear=False, groups=P)
    assert len(got_stats) == P and sum(s["episodes"] for s in got_stats) == env.rollout.episode_stats(clear=False)["episodes"] > 0
    for p in range(P):
        lone_env = hrg.HipVecEnv(m, env_id="ReachHuman", env_kwargs=ek, clips=clips, env_id0=m * p)
        lone_env.attach_rollout(T, gamma=0.99, gae_lambda=0.9)
        lone_env.rollout.generator.manual_seed(seeds[p])   # (the minibatches' permutations: get_groups' generator of group p)
        lone = lone_env.attach_ppo(seed=seeds[p], **kw)
        for _ in range(2):
            lone_env.collect_rollout(lone.policy, lone.value)
            lone.train(lone_env.rollout)
        _assert_member(pop, p, lone, "end to end")
        assert pop.diagnostics()[p] == lone.diagnostics()
        want = lone_env.rollout.export()
        for k in PER_STEP:
            assert np.array_equal(got[k][m * T * p:m * T * (p + 1)], want[k]), (p, k)
        for k in PER_ENV:
            assert np.array_equal(got[k][m * p:m * (p + 1)], want[k]), (p, k)
        assert (got["pos"], got["computed"]) == (want["pos"], want["computed"])
        assert got_stats[p] == lone_env.rollout.episode_stats(clear=False), p
        lone_env.close()
    env.close()
    assert not pop.h.value   # closed with the env


def _resave(src, dst, **changes):
    with np.load(src, allow_pickle=False) as f:
        arrays = {k: f[k] for k in f.files}
    arrays.update(changes)
    np.savez(dst, **arrays)


def test_checkpoints_per_member(tmp_path):
    P, seeds, K, A, B = 2, (11, 12), 6, 4, 32
    kw = dict(net_arch=[dict(pi=[64], vf=[64])], learning_rate=LR, batch_size=B, n_epochs=3, clip_range=0.25, clip_range_vf=0.3, ent_coef=ENT_COEF, log_std_init=-0.5)
    pop = PpoPopulation(K, A, P, seeds, **kw)
    batch = lambda step: _stack([_case(K, A, 1, True, B, 50 + 10 * step + p)[1] for p in range(P)])   # noqa: E731
    one = lambda b, p: RolloutBufferSamples(*(x[p * B:(p + 1) * B].contiguous() for x in b))          # noqa: E731
    pop.step(batch(0))
    pop.policy(torch.zeros(P * 4, K, device="cuda"))
    folder = pop.save(str(tmp_path / "model_final"))
    assert sorted(os.listdir(folder)) == ["member_0.npz", "member_1.npz"]
    loaded, member, again = PpoLearner.load(os.path.join(folder, "member_1.npz")), pop.member(1), PpoPopulation.load(folder)
    assert loaded.desc.seed == member.desc.seed == seeds[1] and again.seeds == list(seeds)
    assert again._hyper() == pop._hyper() == loaded._hyper() == member._hyper() == dict(learning_rate=LR, clip_range=0.25, clip_range_vf=0.3, n_epochs=3)
    assert type(member) is PpoLearner and member.separate and member.batch_size == B
    for name in TENSORS:
        assert torch.equal(getattr(again.p, name), getattr(pop.p, name)), name
    assert again._sizes()[3:5] == pop._sizes()[3:5] == [1, 1] == loaded._sizes()[3:5] == member._sizes()[3:5]
    obs = torch.from_numpy(np.random.RandomState(2).uniform(-1, 1, (P * 5, K)).astype(np.float32)).cuda()
    for step in (1, 2):   # the loaded checkpoint, the member and the two populations continue alike: steps and own draws
        b = batch(step)
        pop.step(b), again.step(b), loaded.step(one(b, 1)), member.step(one(b, 1))
        _assert_member(pop, 1, loaded, f"loaded, step {step}")
        _assert_member(pop, 1, member, f"member, step {step}")
        _assert_member(again, 1, member, f"population loaded, step {step}")
        assert torch.equal(again.p.params, pop.p.params)
        acts = [x.policy(o) for x, o in ((pop, obs), (again, obs), (loaded, obs[5:].contiguous()), (member, obs[5:].contiguous()))]
        assert all(torch.equal(u, w) for u, w in zip(acts[0], acts[1])) and all(torch.equal(u[5:], w) for u, w in zip(acts[0], acts[2]))
        assert all(torch.equal(u, w) for u, w in zip(acts[2], acts[3]))
    # members that are no population: another counter, another clip_range
    for what, changes in (("counters", dict(counters=np.array([2, 1], np.uint64))), ("clip_range", {"hyper.clip_range": np.array(0.2)})):
        other = tmp_path / what
        os.makedirs(other)
        _resave(os.path.join(folder, "member_0.npz"), str(other / "member_0.npz"))
        _resave(os.path.join(folder, "member_1.npz"), str(other / "member_1.npz"), **changes)
        with pytest.raises(ValueError, match=f"member_1.npz: {what} differ from member 0's"):
            PpoPopulation.load(str(other))
    with pytest.raises(ValueError, match="no member_0.npz"):
        PpoPopulation.load(str(tmp_path / "nothing"))
    for h in (pop, again, loaded, member):
        h.close()


def test_evaluate_takes_the_populations_rows():
    P, seeds = 2, (3, 7)
    clips = hrg.synthetic_clips(3, seed=0, min_frames=200, max_frames=300)
    env = hrg.HipVecEnv(8, env_id="ReachHuman", env_kwargs=dict(horizon=10, seed=5), clips=clips)
    env.attach_rollout(8)
    kw = dict(batch_size=32, net_arch=[64, 64], log_std_init=-1.0)
    pop = env.attach_ppo_population(P, seeds=seeds, **kw)
    first = pop.member(0)
    lones = [PpoLearner(pop.obs_dim, pop.act_dim, seed=s, **kw) for s in seeds]
    got = env.evaluate(pop.p.params, 4, learner=first).by_policy()
    stacked = env.evaluate(torch.stack([lone.p.params for lone in lones]), 4, learner=lones[0]).by_policy()
    assert len(got) == len(stacked) == P
    for p, (g, s) in enumerate(zip(got, stacked)):
        assert g.episode_rewards == s.episode_rewards and g.episode_lengths == s.episode_lengths and len(g.episode_rewards) == 4
        assert np.array_equal(g.env, s.env) and np.array_equal(g.step, s.step)
        lone_env = hrg.HipVecEnv(4, env_id="ReachHuman", env_kwargs=dict(horizon=10, seed=5), clips=clips, env_id0=4 * p)   # the lone evaluation on the group's envs
        w = lone_env.evaluate(lones[p], 4)
        assert g.episode_rewards == w.episode_rewards and g.episode_lengths == w.episode_lengths and np.array_equal(g.step, w.step), p
        lone_env.close()
    assert not torch.equal(pop.p.params[0], pop.p.params[1]) and [list(g.policy) for g in got] == [[0] * 4, [1] * 4]   # two policies, a group of envs each
    for h in [first] + lones:
        h.close()
    env.close()


def test_abi_refusals_come_before_anything_is_allocated():
    lib = load_library()
    INVALID, UNSUPPORTED = CONST["HRG_ERR_INVALID"], CONST["HRG_ERR_UNSUPPORTED"]
    err = lambda: lib.hrg_last_error().decode()   # noqa: E731
    desc, seeds, h = build_ppo_desc(6, 4, net_arch=[64], batch_size=32), (ctypes.c_uint64 * 65)(*range(65)), ctypes.c_void_p()
    create = lambda d, n, s: lib.hrg_ppo_population_create(ctypes.byref(d), n, s, 0, ctypes.byref(h))   # noqa: E731
    for n in (0, 65, -3):
        assert create(desc, n, seeds) == UNSUPPORTED and f"n_members = {n} outside 1 .. 64" in err() and not h.value
    assert create(desc, 2, None) == INVALID and "seeds table" in err() and not h.value
    for field, value, code, match in (("hidden", 32, UNSUPPORTED, "hidden = 32"), ("target_kl_set", 1, UNSUPPORTED, "target_kl"), ("batch_size", 48, UNSUPPORTED, "batch_size = 48"),
                                      ("max_grad_norm", 0.0, INVALID, "max_grad_norm")):   # whatever hrg_ppo_create refuses
        bad = build_ppo_desc(6, 4, net_arch=[64], batch_size=32)
        setattr(bad, field, value)
        assert create(bad, 2, seeds) == code and match in err() and not h.value, field
    assert create(desc, 2, seeds) == 0 and h.value
    sizes = (ctypes.c_int64 * 6)()
    assert lib.hrg_ppo_sizes(h, sizes) == 0 and sizes[3] == sizes[4] == 0
    out = torch.zeros(8, 4, device="cuda")
    params = torch.zeros(2, int(sizes[0]), device="cuda")
    forward = lambda n: lib.hrg_ppo_population_forward(h, _ptr(params), _ptr(out), n, None, 1, _ptr(out), _ptr(out), _ptr(out), None)   # noqa: E731
    assert lib.hrg_ppo_forward(h, _ptr(params), _ptr(out), 2, None, 1, _ptr(out), _ptr(out), _ptr(out), None) == INVALID and "hrg_ppo_population_forward" in err()
    assert forward(0) == INVALID and "n must be positive" in err() and forward(-1) == INVALID
    assert lib.hrg_ppo_population_forward(h, _ptr(params), _ptr(out), 2, None, 1, _ptr(out), _ptr(out), None, None) == INVALID and "without log_probs" in err()
    assert lib.hrg_ppo_population_export(h, 2, None, None, None, None, None) == INVALID and "member = 2" in err()
    assert lib.hrg_ppo_population_export(h, -1, None, None, None, None, None) == INVALID
    assert lib.hrg_ppo_population_export(h, 1, None, None, None, None, None) == 0
    assert lib.hrg_ppo_sizes(h, sizes) == 0 and sizes[3] == sizes[4] == 0   # nothing ran
    lib.hrg_ppo_destroy(h)
