"""Hyper-parameters per member of a SAC population (csrc/hrgym_sac.h): the step kernels read learning rate, gamma, tau, target entropy and the
entropy coefficient's fixed value and learned flag from the member's row of a device table.  -m gpu.

The specification is exact: member p equals, bit for bit, the lone SacLearner constructed with member p's seed and values on member p's rows -- the row is
read once per workgroup and used in the lone learner's types and order.  Every comparison is torch.equal on tensors and equality of the uint32 views of the
exports; there is no tolerance."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import human_robot_gym_amd as hrg
from human_robot_gym_amd._cstruct import CONST, SacHyper
from human_robot_gym_amd._learner import MANIFEST, TENSORS, read_manifest
from human_robot_gym_amd._lib import load_library
from human_robot_gym_amd.replay import ReplayBufferSamples
from human_robot_gym_amd.sac import SacLearner, SacPopulation, build_sac_desc

pytestmark = pytest.mark.gpu

K, A, B = 6, 4, CONST["HRG_SAC_TILE"]
SEEDS = (5, 9, 2)
EXPORT_KEYS = ("y", "logp", "logp_next", "q", "grad", "losses")
# every field distinct across the members; member 1's coefficient is fixed, member 2's target entropy is its own
VALUES = dict(learning_rate=[1e-3, 3e-4, 1e-4], gamma=[0.99, 0.9, 0.95], tau=[0.005, 0.05, 0.5], ent_coef=["auto_0.2", 0.1, "auto"], target_entropy=["auto", "auto", -2.0])


def _shared(depth):
    return dict(net_arch=[64] * depth, batch_size=B, target_update_interval=2)


def _of(values, p):
    return {k: v[p] for k, v in values.items()}



def _batches(P, steps, seed):
    """`steps` batches of P * B fixed random rows."""
    rng = np.random.RandomState(seed)
    f = lambda *shape: torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32)).cuda()   # noqa: E731
    out = []
    for _ in range(steps):
        done = torch.from_numpy((rng.uniform(size=(P * B, 1)) < 0.2).astype(np.float32)).cuda()
        out.append(ReplayBufferSamples(observations=f(P * B, K), actions=f(P * B, A), next_observations=f(P * B, K), dones=done, rewards=f(P * B, 1)))
    return out


def _slice(batch, p):
    return ReplayBufferSamples(*(x[p * B:(p + 1) * B].contiguous() for x in batch))


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _assert_member(pop, p, lone, what):
    for name in TENSORS:
        assert torch.equal(getattr(pop.p, name)[p], getattr(lone.p, name)), (what, p, name)
    got, want = pop.export(member=p), lone.export()
    for k in EXPORT_KEYS:
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (what, p, k)
    assert pop._sizes()[3:5] == lone._sizes()[3:5], (what, p, "counters")


def _lones(values, P, depth):
    return [SacLearner(K, A, seed=SEEDS[p], **_shared(depth), **_of(values, p)) for p in range(P)]


def _close(*handles):
    for h in handles:
        h.close()


def _pick(values, members):
    return {k: [v[m] for m in members] for k, v in values.items()}


@pytest.mark.parametrize("members, depth", [((0, 1, 2), 1), ((1, 2), 3)])   # P = 3 at depth 1, P = 2 at depth 3; every field distinct across the members in both
def test_a_member_is_the_lone_learner_of_its_values(members, depth):
    P, values = len(members), _pick(VALUES, members)
    fixed, learned = members.index(1), members.index(2)   # the member of the fixed coefficient, one of a learned one
    pop = SacPopulation(K, A, P, SEEDS[:P], **_shared(depth), **values)
    lones = _lones(values, P, depth)
    assert pop.varying() == list(VALUES) and pop._per_member and [pop.member_hyper(p) for p in range(P)] == [_of(values, p) for p in range(P)]
    coef = pop.p.n_params - 1   # log_ent_coef
    assert [float(pop.p.params[p, coef]) for p in range(P)] == [np.float32(math.log((0.2, 0.1, 1.0)[m])) for m in members]   # row p follows member p's ent_coef
    for step, batch in enumerate(_batches(P, 3, 17 * P + depth)):   # three steps: Adam's bias correction, both phases of the target update, the coefficient's Adam step
        pop.step(batch)
        for p, lone in enumerate(lones):
            lone.step(_slice(batch, p))
            _assert_member(pop, p, lone, f"step {step}")
        # the fixed member's coefficient entry gets no gradient and no Adam step
        assert float(pop.p.params[fixed, coef]) == np.float32(math.log(0.1)) and float(pop.p.adam_m[fixed, coef]) == 0.0 == float(pop.p.adam_v[fixed, coef])
        assert float(pop.p.params[learned, coef]) != 0.0 and float(pop.p.adam_v[learned, coef]) > 0.0   # (the learned one, from log 1, moves)
    diag = pop.diagnostics()
    assert all(d == lone.diagnostics() for d, lone in zip(diag, lones)) and diag[fixed]["ent_coef"] == float(np.float32(0.1)) and diag[fixed]["ent_coef_loss"] == 0.0
    _close(pop, *lones)


def test_a_members_row_reaches_no_other_member():
    P, depth = 3, 1
    changed = {k: list(v) for k, v in VALUES.items()}
    for k, v in dict(learning_rate=5e-4, gamma=0.8, tau=0.2, ent_coef="auto_0.3", target_entropy=-1.0).items():
        changed[k][1] = v
    batches = _batches(P, 3, 3)
    runs = []
    for values in (VALUES, changed):
        pop = SacPopulation(K, A, P, SEEDS, **_shared(depth), **values)
        for batch in batches:
            pop.step(batch)
        runs.append(({name: getattr(pop.p, name).clone() for name in TENSORS}, [pop.export(member=p) for p in range(P)]))
        pop.close()
    (t0, e0), (t1, e1) = runs
    for p in (0, 2):
        assert all(torch.equal(t0[name][p], t1[name][p]) for name in TENSORS), p
        assert all(np.array_equal(_bits(e0[p][k]), _bits(e1[p][k])) for k in EXPORT_KEYS), p
    assert not torch.equal(t0["params"][1], t1["params"][1]) and not torch.equal(t0["target"][1], t1["target"][1])
    assert not np.array_equal(e0[1]["y"], e1[1]["y"])


def test_equal_values_per_member_are_the_scalar_population():
    P, depth, lr = 3, 1, 5e-4
    scalar = dict(learning_rate=lr, gamma=0.97, tau=0.01, ent_coef="auto_0.2", target_entropy=-3.0)
    one = SacPopulation(K, A, P, SEEDS, **_shared(depth), **scalar)
    many = SacPopulation(K, A, P, SEEDS, **_shared(depth), **{k: [v] * P for k, v in scalar.items()})
    assert one._hyper() == many._hyper() == dict(learning_rate=lr) and many.varying() == [] and not many._per_member and many.learning_rate == lr
    for batch in _batches(P, 3, 4):
        one.step(batch), many.step(batch)
        for name in TENSORS:
            assert torch.equal(getattr(one.p, name), getattr(many.p, name)), name
    table = SacPopulation(K, A, P, SEEDS, **_shared(depth), **scalar)   # the same values through an uploaded table
    table._per_member = True
    table._sync_table()
    for batch in _batches(P, 3, 4):
        table.step(batch)
    for name in TENSORS:
        assert torch.equal(getattr(one.p, name), getattr(table.p, name)), name
    _close(one, many, table)


def test_a_learning_rate_per_member_between_two_steps():
    P, depth = 3, 1
    values = dict(VALUES, learning_rate=7e-4)
    pop = SacPopulation(K, A, P, SEEDS, **_shared(depth), **values)
    lones = [SacLearner(K, A, seed=SEEDS[p], **_shared(depth), **{k: (v[p] if isinstance(v, list) else v) for k, v in values.items()}) for p in range(P)]
    new = [2e-3, 5e-4, 0.0]
    for step, batch in enumerate(_batches(P, 3, 8)):
        if step == 1:
            pop.learning_rate = new
            for lone, lr in zip(lones, new):
                lone.learning_rate = lr
            assert pop.learning_rate == new and pop._hyper() == dict(learning_rate=new) and [pop.member_hyper(p)["learning_rate"] for p in range(P)] == new
        pop.step(batch)
        for p, lone in enumerate(lones):
            lone.step(_slice(batch, p))
            _assert_member(pop, p, lone, f"step {step}")
    pop.learning_rate = 1e-3   # a scalar again: every member
    assert pop.learning_rate == 1e-3 and pop._hyper() == dict(learning_rate=1e-3)
    with pytest.raises(ValueError, match="learning_rate: 2 values for 3 members"):
        pop.learning_rate = [1e-3, 1e-4]
    with pytest.raises(ValueError, match="learning_rate"):
        pop.learning_rate = [1e-3, 1e-4, -1.0]
    assert pop.learning_rate == 1e-3
    _close(pop, *lones)


def test_checkpoints_carry_each_members_values(tmp_path):
    P, depth = 3, 1
    pop = SacPopulation(K, A, P, SEEDS, **_shared(depth), **VALUES)
    batches = _batches(P, 3, 12)
    pop.step(batches[0])
    pop.act(torch.zeros(P * 4, K, device="cuda"))
    folder = pop.save(str(tmp_path / "model_final"))
    assert sorted(os.listdir(folder)) == [f"member_{p}.npz" for p in range(P)] + [MANIFEST]
    assert read_manifest(folder, "hrg_sac") == ("auto_ent_coef", "ent_coef", "gamma", "learning_rate", "target_entropy", "tau")
    with np.load(os.path.join(folder, MANIFEST), allow_pickle=False) as f:
        assert all(f[k].dtype != object for k in f.files)
    loaded, member, again = SacLearner.load(os.path.join(folder, "member_1.npz")), pop.member(1), SacPopulation.load(folder)
    for lone in (loaded, member):
        assert type(lone) is SacLearner and lone.desc.seed == SEEDS[1] and not lone.auto_ent_coef
        assert (lone.learning_rate, lone.desc.gamma, lone.desc.tau, lone.desc.ent_coef, lone.desc.target_entropy) == (3e-4, 0.9, 0.05, 0.1, -4.0)
    assert again.seeds == list(SEEDS) and again.learning_rate == VALUES["learning_rate"] and again._per_member
    assert [again.member_hyper(p)["gamma"] for p in range(P)] == VALUES["gamma"] and again.member_hyper(1)["ent_coef"] == 0.1
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
        SacPopulation.load(folder)
    _close(pop, again, loaded, member)


def test_set_hyper_refuses_before_anything_is_written():
    lib = load_library()
    INVALID = CONST["HRG_ERR_INVALID"]
    err = lambda: lib.hrg_last_error().decode()   # noqa: E731
    P, depth = 3, 1
    pop = SacPopulation(K, A, P, SEEDS, **_shared(depth), **VALUES)
    twin = SacPopulation(K, A, P, SEEDS, **_shared(depth), **VALUES)   # never sees a refused table
    rows = lambda: (SacHyper * P)(*(pop._row(p) for p in range(P)))   # noqa: E731
    set_hyper = lambda table, n=P: lib.hrg_sac_population_set_hyper(pop.h, table, n, pop._stream())   # noqa: E731
    batches = _batches(P, 6, 21)

    def still_steps(batch):
        pop.step(batch), twin.step(batch)
        for name in TENSORS:
            assert torch.equal(getattr(pop.p, name), getattr(twin.p, name)), name

    assert set_hyper(None) == INVALID and "null" in err()
    still_steps(batches[0])
    assert set_hyper(ctypes.byref(rows()), 2) == INVALID and "n_members = 2" in err() and "3 members" in err()
    still_steps(batches[1])
    for k, (field, value) in enumerate((("tau", 1.5), ("gamma", float("nan")), ("learning_rate", -1e-3))):
        bad = rows()
        bad[0].learning_rate, bad[2].gamma = 0.5, 0.5   # valid rows around the refused one: written only if the entry does not check first
        setattr(bad[1], field, value)
        assert set_hyper(ctypes.byref(bad)) == INVALID and "member 1" in err() and field in err(), (field, err())
        still_steps(batches[2 + k])
    bad = rows()
    bad[2].auto_ent_coef, bad[2].ent_coef = 0, 0.0
    assert set_hyper(ctypes.byref(bad)) == INVALID and "member 2" in err() and "ent_coef" in err()
    assert set_hyper(ctypes.byref(rows())) == 0   # the table again, as it was
    still_steps(batches[5])
    h = ctypes.c_void_p()   # the lone learner's handle takes a table of one row
    assert lib.hrg_sac_create(ctypes.byref(build_sac_desc(K, A, batch_size=B)), 0, ctypes.byref(h)) == 0
    assert lib.hrg_sac_population_set_hyper(h, ctypes.byref(rows()), P, None) == INVALID and "n_members = 3" in err()
    assert lib.hrg_sac_population_set_hyper(h, ctypes.byref(rows()), 1, None) == 0
    lib.hrg_sac_destroy(h)
    _close(pop, twin)


def test_through_the_env_a_learning_rate_per_member():
    P, m, lrs = 3, 4, [1e-3, 3e-4, 1e-4]
    kw = dict(batch_size=B, ent_coef="auto_0.2", net_arch=[64, 64])
    clips = hrg.synthetic_clips(3, seed=0, min_frames=200, max_frames=300)
    ek = dict(horizon=6, seed=5)
    env = hrg.HipVecEnv(P * m, env_id="ReachHuman", env_kwargs=ek, clips=clips)
    env.attach_replay(P * m * 20)
    with pytest.raises(NotImplementedError, match="batch_size = .*one value per member is not supported"):
        env.attach_sac_population(P, seeds=[0, 0, 0], **dict(kw, batch_size=[32, 32, 64]))
    with pytest.raises(ValueError, match="learning_rate: 2 values for 3 members"):
        env.attach_sac_population(P, seeds=[0, 0, 0], learning_rate=lrs[:2], **kw)
    assert env.sac_population is None
    pop = env.attach_sac_population(P, seeds=[0, 0, 0], learning_rate=lrs, **kw)
    assert env.sac_population is pop and pop.learning_rate == lrs and pop.varying() == ["learning_rate"]
    env.collect_steps(pop.act, 8)
    pop.train(env.replay, 2)
    for p, q in ((0, 1), (0, 2), (1, 2)):   # one seed, one distribution of the data, three learning rates
        assert not torch.equal(pop.p.params[p], pop.p.params[q]), (p, q)
    lone_env = hrg.HipVecEnv(m, env_id="ReachHuman", env_kwargs=ek, clips=clips, env_id0=0)   # member 0's group as a run of its own
    lone_env.attach_replay(m * 20, seed=0)
    lone = lone_env.attach_sac(seed=0, learning_rate=lrs[0], **kw)
    lone_env.collect_steps(lone.act, 8)
    lone.train(lone_env.replay, 2)
    _assert_member(pop, 0, lone, "end to end")
    assert [d["n_updates"] for d in pop.diagnostics()] == [2, 2, 2]
    lone_env.close()
    env.close()
