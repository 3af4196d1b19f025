"""Hyper-parameters per member of a PPO population (csrc/hrgym_ppo.h): the step kernels read learning rate, the two clip ranges, ent_coef, vf_coef
and max_grad_norm from the member's row of a device table.  -m gpu.

The specification is exact: member p equals, bit for bit, the lone PpoLearner constructed with member p's seed and values on member p's rows.  Every comparison
is torch.equal on tensors and equality of the uint32 views of the exports, `diag` included; there is no tolerance."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import human_robot_gym_amd as hrg
from human_robot_gym_amd._cstruct import CONST, PpoHyper
from human_robot_gym_amd._learner import MANIFEST, read_manifest
from human_robot_gym_amd._lib import load_library
from human_robot_gym_amd.ppo import DIAG_KEYS, PpoLearner, PpoPopulation, build_ppo_desc
from human_robot_gym_amd.rollout import RolloutBufferSamples

pytestmark = pytest.mark.gpu

K, A, B, P = 6, 4, CONST["HRG_PPO_TILE"], 3
SEEDS = (5, 9, 2)
TENSORS = ("params", "adam_m", "adam_v")
ARCHS = dict(shared=[64], separate=[dict(pi=[64, 64], vf=[64, 64])])
# every field distinct across the members.  max_grad_norm: member 1's gradient is clipped at every step, member 2's at none (asserted from the lone learners'
# exported grad_norm below)
VALUES = dict(learning_rate=[1e-3, 3e-4, 1e-4], clip_range=[0.2, 0.1, 0.3], clip_range_vf=[None, 0.3, 0.1], ent_coef=[0.0, 0.01, 0.001], vf_coef=[0.5, 0.25, 1.0],
              max_grad_norm=[0.5, 1e-3, 1e3])


def _shared(arch):
    return dict(net_arch=ARCHS[arch], batch_size=B, log_std_init=-0.5)


def _of(values, p):
    return {k: (v[p] if isinstance(v, list) else v) for k, v in values.items()}


@functools.lru_cache(maxsize=None)
def _batches(arch, steps, seed):
    """`steps` minibatches of P * B fixed random rows; computed once, shared and left unchanged.  Old values and log probabilities are those of the members'
    initial networks (the same for every population of SEEDS here) moved by noise as wide as the clip ranges, so that rows fall on both sides of each of them."""
    pop = PpoPopulation(K, A, P, SEEDS, **_shared(arch))
    g = torch.Generator().manual_seed(seed)
    f = lambda *shape: torch.randn(*shape, generator=g).cuda()   # noqa: E731
    out = []
    for _ in range(steps):
        obs = f(P * B, K)
        actions, values, log_probs = pop.policy(obs, eps=f(P * B, A))   # (supplied noise: the forward counter stays)
        out.append(RolloutBufferSamples(obs, actions, (values + 0.3 * f(P * B)).contiguous(), (log_probs + 0.3 * f(P * B)).contiguous(), f(P * B) + 0.3, values + f(P * B)))
    pop.close()
    return tuple(out)


def _slice(batch, p):
    return RolloutBufferSamples(*(x[p * B:(p + 1) * B].contiguous() for x in batch))


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _assert_member(pop, p, lone, what):
    for name in TENSORS:
        assert torch.equal(getattr(pop.p, name)[p], getattr(lone.p, name)), (what, p, name)
    got, want = pop.export(member=p), lone.export()
    for k in ("values", "log_prob", "ratio", "grad"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (what, p, k)
    assert _bits(np.array([got["diag"][k] for k in DIAG_KEYS], np.float32)).tolist() == _bits(np.array([want["diag"][k] for k in DIAG_KEYS], np.float32)).tolist(), (what, p, "diag")
    assert pop._sizes()[3:5] == lone._sizes()[3:5], (what, p, "counters")


def _lones(values, arch):
    return [PpoLearner(K, A, seed=SEEDS[p], **_shared(arch), **_of(values, p)) for p in range(P)]


def _close(*handles):
    for h in handles:
        h.close()


@pytest.mark.parametrize("arch", list(ARCHS))
def test_a_member_is_the_lone_learner_of_its_values(arch):
    pop = PpoPopulation(K, A, P, SEEDS, **_shared(arch), **VALUES)
    lones = _lones(VALUES, arch)
    assert pop.varying() == list(VALUES) and pop._per_member and [pop.member_hyper(p) for p in range(P)] == [_of(VALUES, p) for p in range(P)]
    for step, batch in enumerate(_batches(arch, 3, 7)):
        pop.step(batch)
        for p, lone in enumerate(lones):
            lone.step(_slice(batch, p))
            _assert_member(pop, p, lone, f"step {step}")
        diag = [lone.export()["diag"] for lone in lones]
        assert diag[1]["grad_norm"] > VALUES["max_grad_norm"][1] and diag[2]["grad_norm"] < VALUES["max_grad_norm"][2], (step, diag)   # one clipped, one not
        assert all(0.0 < d["clip_fraction"] < 1.0 for d in diag), (step, diag)   # rows on both sides of every member's clip_range
    diag = pop.diagnostics()
    assert all(d == lone.diagnostics() for d, lone in zip(diag, lones))
    assert [d["clip_range"] for d in diag] == VALUES["clip_range"] and [d["learning_rate"] for d in diag] == VALUES["learning_rate"]
    assert [d.get("clip_range_vf") for d in diag] == VALUES["clip_range_vf"]
    _close(pop, *lones)


def test_a_members_row_reaches_no_other_member():
    arch = "shared"
    changed = {k: list(v) for k, v in VALUES.items()}
    for k, v in dict(learning_rate=5e-4, clip_range=0.15, clip_range_vf=None, ent_coef=0.02, vf_coef=0.75, max_grad_norm=0.01).items():
        changed[k][1] = v
    runs = []
    for values in (VALUES, changed):
        pop = PpoPopulation(K, A, P, SEEDS, **_shared(arch), **values)
        for batch in _batches(arch, 3, 7):
            pop.step(batch)
        runs.append(({name: getattr(pop.p, name).clone() for name in TENSORS}, [pop.export(member=p) for p in range(P)]))
        pop.close()
    (t0, e0), (t1, e1) = runs
    for p in (0, 2):
        assert all(torch.equal(t0[name][p], t1[name][p]) for name in TENSORS), p
        assert all(np.array_equal(_bits(e0[p][k]), _bits(e1[p][k])) for k in ("values", "log_prob", "ratio", "grad")) and e0[p]["diag"] == e1[p]["diag"], p
    assert not torch.equal(t0["params"][1], t1["params"][1]) and e0[1]["diag"] != e1[1]["diag"]


def test_equal_values_per_member_are_the_scalar_population():
    arch = "shared"
    scalar = dict(learning_rate=5e-4, clip_range=0.25, clip_range_vf=0.2, ent_coef=0.01, vf_coef=0.4, max_grad_norm=0.3)
    one = PpoPopulation(K, A, P, SEEDS, n_epochs=3, **_shared(arch), **scalar)
    many = PpoPopulation(K, A, P, SEEDS, n_epochs=3, **_shared(arch), **{k: [v] * P for k, v in scalar.items()})
    assert one._hyper() == many._hyper() == dict(learning_rate=5e-4, clip_range=0.25, clip_range_vf=0.2, n_epochs=3) and many.varying() == [] and not many._per_member
    table = PpoPopulation(K, A, P, SEEDS, n_epochs=3, **_shared(arch), **scalar)   # the same values through an uploaded table
    table._per_member = True
    table._sync_table()
    for batch in _batches(arch, 3, 7):
        one.step(batch), many.step(batch), table.step(batch)
        for name in TENSORS:
            assert torch.equal(getattr(one.p, name), getattr(many.p, name)) and torch.equal(getattr(one.p, name), getattr(table.p, name)), name
    _close(one, many, table)


def test_scheduled_attributes_per_member_between_two_steps():
    arch = "shared"
    values = dict(VALUES, learning_rate=7e-4, clip_range=0.2, clip_range_vf=None)
    pop = PpoPopulation(K, A, P, SEEDS, **_shared(arch), **values)
    lones = _lones(values, arch)
    new = dict(learning_rate=[2e-3, 5e-4, 0.0], clip_range=[0.3, 0.2, 0.1], clip_range_vf=[0.2, None, 0.4])
    for step, batch in enumerate(_batches(arch, 3, 7)):
        if step == 1:
            for name, vals in new.items():
                setattr(pop, name, vals)
                for lone, v in zip(lones, vals):
                    setattr(lone, name, v)
            assert pop._hyper() == dict(new, n_epochs=10) and [pop.member_hyper(p)["clip_range_vf"] for p in range(P)] == new["clip_range_vf"]
        pop.step(batch)
        for p, lone in enumerate(lones):
            lone.step(_slice(batch, p))
            _assert_member(pop, p, lone, f"step {step}")
    pop.clip_range = 0.2   # a scalar again: every member
    assert pop.clip_range == 0.2 and pop._hyper()["clip_range"] == 0.2
    with pytest.raises(ValueError, match="clip_range: 2 values for 3 members"):
        pop.clip_range = [0.1, 0.2]
    with pytest.raises(ValueError, match="clip_range_vf"):
        pop.clip_range_vf = [None, 0.1, 0.0]
    assert pop.clip_range == 0.2 and pop.clip_range_vf == new["clip_range_vf"]
    _close(pop, *lones)


def test_checkpoints_carry_each_members_values(tmp_path):
    arch = "separate"
    pop = PpoPopulation(K, A, P, SEEDS, n_epochs=3, **_shared(arch), **VALUES)
    batches = _batches(arch, 3, 7)
    pop.step(batches[0])
    pop.policy(torch.zeros(P * 4, K, device="cuda"))
    folder = pop.save(str(tmp_path / "model_final"))
    assert sorted(os.listdir(folder)) == [f"member_{p}.npz" for p in range(P)] + [MANIFEST]
    assert read_manifest(folder, "hrg_ppo") == tuple(sorted(VALUES))
    with np.load(os.path.join(folder, MANIFEST), allow_pickle=False) as f:
        assert all(f[k].dtype != object for k in f.files)
    loaded, member, again = PpoLearner.load(os.path.join(folder, "member_1.npz")), pop.member(1), PpoPopulation.load(folder)
    for lone in (loaded, member):
        assert type(lone) is PpoLearner and lone.desc.seed == SEEDS[1] and lone._hyper() == dict(learning_rate=3e-4, clip_range=0.1, clip_range_vf=0.3, n_epochs=3)
        assert (lone.desc.ent_coef, lone.desc.vf_coef, lone.desc.max_grad_norm) == (0.01, 0.25, 1e-3)
    assert again.seeds == list(SEEDS) and again._per_member and [again.member_hyper(p) for p in range(P)] == [_of(VALUES, p) for p in range(P)] and again.n_epochs == 3
    for name in TENSORS:
        assert torch.equal(getattr(again.p, name), getattr(pop.p, name)), name
    assert again._sizes()[3:5] == pop._sizes()[3:5] == [1, 1] == loaded._sizes()[3:5] == member._sizes()[3:5]
    for step, batch in enumerate(batches[1:]):   # the loaded population, the loaded member and member(1) continue alike, two more steps
        pop.step(batch), again.step(batch), loaded.step(_slice(batch, 1)), member.step(_slice(batch, 1))
        for name in TENSORS:
            assert torch.equal(getattr(again.p, name), getattr(pop.p, name)), (step, name)
        _assert_member(pop, 1, loaded, f"loaded, step {step}")
        _assert_member(pop, 1, member, f"member, step {step}")
    os.remove(os.path.join(folder, MANIFEST))   # without the manifest the members are no population, in the words of before
    with pytest.raises(ValueError, match="member_1.npz: .*differ from member 0's: the members of a population share them"):
        PpoPopulation.load(folder)
    _close(pop, again, loaded, member)


def test_set_hyper_refuses_before_anything_is_written():
    lib = load_library()
    INVALID = CONST["HRG_ERR_INVALID"]
    err = lambda: lib.hrg_last_error().decode()   # noqa: E731
    arch = "shared"
    pop = PpoPopulation(K, A, P, SEEDS, **_shared(arch), **VALUES)
    twin = PpoPopulation(K, A, P, SEEDS, **_shared(arch), **VALUES)   # never sees a refused table
    rows = lambda: (PpoHyper * P)(*(pop._row(p) for p in range(P)))   # noqa: E731
    set_hyper = lambda table, n=P: lib.hrg_ppo_population_set_hyper(pop.h, table, n, pop._stream())   # noqa: E731
    batches = _batches(arch, 3, 7) + _batches(arch, 3, 8) + _batches(arch, 3, 9)

    def still_steps(batch):
        pop.step(batch), twin.step(batch)
        for name in TENSORS:
            assert torch.equal(getattr(pop.p, name), getattr(twin.p, name)), name

    assert set_hyper(None) == INVALID and "null" in err()
    still_steps(batches[0])
    assert set_hyper(ctypes.byref(rows()), 2) == INVALID and "n_members = 2" in err() and "3 members" in err()
    still_steps(batches[1])
    cases = (("learning_rate", -1e-3), ("clip_range", 0.0), ("clip_range_vf", float("nan")), ("ent_coef", float("inf")), ("vf_coef", -0.5), ("max_grad_norm", 0.0))
    for k, (field, value) in enumerate(cases):
        bad = rows()
        bad[0].learning_rate, bad[2].clip_range = 0.5, 0.5   # valid rows around the refused one: written only if the entry does not check first
        setattr(bad[1], field, value)
        assert set_hyper(ctypes.byref(bad)) == INVALID and "member 1" in err() and field + " =" in err(), (field, err())
        still_steps(batches[2 + k])
    assert set_hyper(ctypes.byref(rows())) == 0   # the table again, as it was
    still_steps(batches[8])
    h = ctypes.c_void_p()   # the lone learner's handle takes a table of one row
    assert lib.hrg_ppo_create(ctypes.byref(build_ppo_desc(K, A, net_arch=[64], batch_size=B)), 0, ctypes.byref(h)) == 0
    assert lib.hrg_ppo_population_set_hyper(h, ctypes.byref(rows()), P, None) == INVALID and "n_members = 3" in err()
    assert lib.hrg_ppo_population_set_hyper(h, ctypes.byref(rows()), 1, None) == 0
    lib.hrg_ppo_destroy(h)
    _close(pop, twin)


def test_through_the_env_a_clip_range_per_member():
    m, T, clips_range = 4, 8, [0.1, 0.2, 0.3]
    kw = dict(batch_size=32, n_epochs=2, learning_rate=1e-3, net_arch=[64, 64], log_std_init=-1.0, ortho_init=False)
    clips = hrg.synthetic_clips(3, seed=0, min_frames=200, max_frames=300)
    ek = dict(horizon=6, seed=5)
    env = hrg.HipVecEnv(P * m, env_id="ReachHuman", env_kwargs=ek, clips=clips)
    env.attach_rollout(T, gamma=0.99, gae_lambda=0.9)
    with pytest.raises(NotImplementedError, match="batch_size = .*one value per member is not supported"):
        env.attach_ppo_population(P, seeds=[0, 0, 0], **dict(kw, batch_size=[32, 32, 16]))
    with pytest.raises(ValueError, match="clip_range: 2 values for 3 members"):
        env.attach_ppo_population(P, seeds=[0, 0, 0], clip_range=clips_range[:2], **kw)
    assert env.ppo_population is None
    pop = env.attach_ppo_population(P, seeds=[0, 0, 0], clip_range=clips_range, **kw)
    assert env.ppo_population is pop and pop.clip_range == clips_range and pop.varying() == ["clip_range"] and pop.desc.rollout_size == m * T
    env.collect_rollout(pop.policy, pop.value)
    pop.train(env.rollout)
    assert pop.n_updates == 2 * (m * T // 32)
    for p, q in ((0, 1), (0, 2), (1, 2)):   # one seed, three clip ranges
        assert not torch.equal(pop.p.params[p], pop.p.params[q]), (p, q)
    lone_env = hrg.HipVecEnv(m, env_id="ReachHuman", env_kwargs=ek, clips=clips, env_id0=0)   # member 0's group as a run of its own
    lone_env.attach_rollout(T, gamma=0.99, gae_lambda=0.9)
    lone_env.rollout.generator.manual_seed(0)   # (the minibatches' permutations: get_groups' generator of group 0)
    lone = lone_env.attach_ppo(seed=0, clip_range=clips_range[0], **kw)
    lone_env.collect_rollout(lone.policy, lone.value)
    lone.train(lone_env.rollout)
    _assert_member(pop, 0, lone, "end to end")
    assert pop.diagnostics()[0] == lone.diagnostics() and [d["clip_range"] for d in pop.diagnostics()] == clips_range
    lone_env.close()
    env.close()
