"""The PPO population, host side: the seeds table and the stacked tensors, the refusals that come before the device is touched, the ABI, the index arithmetic
of the grouped minibatches and the tool's parser.  No GPU.  What a member computes is tests/test_ppo_population_gpu.py's."""
import ctypes
import importlib.util
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import human_robot_gym_amd as hrg
from helpers import OracleBackend
from human_robot_gym_amd import _learner, ppo, rollout, sac
from human_robot_gym_amd._cstruct import CONST, PROTOTYPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_seeds_table_is_the_one_both_populations_share():
    assert CONST["HRG_PPO_MAX_POPULATION"] == ppo.MAX_POPULATION == 64
    assert ppo.check_seeds is sac.check_seeds is _learner.check_seeds   # written once; importable under its earlier name
    P, table = ppo.check_seeds(3, (5, 9, -1))
    assert P == 3 and table.dtype == np.uint64 and table.tolist() == [5, 9, 2**64 - 1]   # (a seed is its low 64 bits, as build_ppo_desc keeps it)
    d = ppo.build_ppo_desc(6, 4, net_arch=[64], batch_size=64, seed=9)
    assert ctypes.sizeof(d) == 12 * 4 + 3 * 8 + 8   # the descriptor a population shares is the lone learner's, unchanged
    assert issubclass(ppo.PpoPopulation, ppo.PpoLearner) and issubclass(ppo.PpoPopulation, _learner.Population) and issubclass(sac.SacPopulation, _learner.Population)
    assert hrg.PpoPopulation is ppo.PpoPopulation


@pytest.mark.parametrize("P", [0, 65, -1])
def test_members_outside_the_range_are_refused(P):
    with pytest.raises(NotImplementedError, match=f"n_members = {P}"):   # before the device or the library is touched
        ppo.PpoPopulation(6, 4, P, list(range(max(P, 0))), net_arch=[64], batch_size=64)


def test_wrong_number_of_seeds_and_whatever_the_lone_learner_refuses():
    with pytest.raises(ValueError, match="2 seeds for 3 members"):
        ppo.PpoPopulation(6, 4, 3, [1, 2], net_arch=[64], batch_size=64)
    with pytest.raises(NotImplementedError, match="batch_size = 48"):
        ppo.PpoPopulation(6, 4, 2, [1, 2], net_arch=[64], batch_size=48)
    with pytest.raises(NotImplementedError, match="net_arch"):
        ppo.PpoPopulation(6, 4, 2, [1, 2], net_arch=[32], batch_size=64)
    with pytest.raises(NotImplementedError, match="target_kl"):
        ppo.PpoPopulation(6, 4, 2, [1, 2], net_arch=[64], batch_size=64, target_kl=0.01)
    with pytest.raises(NotImplementedError, match="no short last minibatch"):
        ppo.PpoPopulation(6, 4, 2, [1, 2], net_arch=[64], batch_size=64, rollout_size=96)
    with pytest.raises(NotImplementedError, match="policy_kwargs"):
        ppo.PpoPopulation(6, 4, 2, [1, 2], net_arch=[64], batch_size=64, sde_net_arch=[8])
    with pytest.raises(ValueError, match="n_epochs"):
        ppo.PpoPopulation(6, 4, 2, [1, 2], net_arch=[64], batch_size=64, n_epochs=0)


@pytest.mark.parametrize("depth, separate, ortho", [(2, True, True), (1, False, False)])
def test_parameter_rows_are_the_lone_learners_initialisation(depth, separate, ortho):
    seeds = (5, 9, 2)
    pop = ppo.PpoPopulationParams(6, 4, depth, separate, seeds, log_std_init=-2.7, ortho_init=ortho)
    n = ppo.param_layout(6, 4, depth, separate)[1]
    assert tuple(pop.params.shape) == tuple(pop.adam_m.shape) == tuple(pop.adam_v.shape) == (3, n) and pop.n_params == n and not hasattr(pop, "target")
    for p, s in enumerate(seeds):
        lone = ppo.PpoParams(6, 4, depth, separate, seed=s, log_std_init=-2.7, ortho_init=ortho)
        assert torch.equal(pop.params[p], lone.params) and list(pop.layout) == list(lone.layout)
        assert not pop.adam_m[p].any() and not pop.adam_v[p].any()
        m = pop.member(p)
        assert sorted(vars(m)) == ["adam_m", "adam_v", "params"]
        assert m.params.data_ptr() == pop.params[p].data_ptr() and m.adam_v.is_contiguous()   # views: a checkpoint restored into them lands in the rows
    assert not torch.equal(pop.params[0], pop.params[1])
    assert bool((pop.params[:, -4:] == np.float32(-2.7)).all())


def _oracle_env(n, **kw):
    clips = hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300)
    ek = dict(shield_type="OFF", horizon=5)
    return hrg.HipVecEnv(n, env_kwargs=ek, clips=clips, backend=OracleBackend(hrg.build_model_desc(ek, n_clips=2), clips, n), **kw)


def test_attach_refusals_by_name():
    env = _oracle_env(3)
    assert env.ppo_population is None
    with pytest.raises(NotImplementedError, match="n_members = 65"):
        env.attach_ppo_population(65)
    with pytest.raises(NotImplementedError, match="n_members = 0"):
        env.attach_ppo_population(0)
    with pytest.raises(ValueError, match="1 seeds for 3 members"):
        env.attach_ppo_population(3, seeds=[4])
    with pytest.raises(TypeError, match="seeds"):
        env.attach_ppo_population(3, seed=4)
    with pytest.raises(NotImplementedError, match="attach_ppo_population: the rollout kernels run in the HIP library"):   # another backend
        env.attach_ppo_population(3)
    # an env that could carry a buffer and has none: the oracle env with its backend's refusal lifted (the device is not reached: the buffer is looked at first)
    env.device_refusal = lambda kind: None
    with pytest.raises(NotImplementedError, match=r"attach_ppo_population: call attach_rollout\(n_steps, gamma, gae_lambda\) first"):
        env.attach_ppo_population(3)
    # ... and with a buffer's sizes in its place: the groups and the minibatches are checked before a learner is made
    env._device_path.buffers["rollout"] = NS(n=3, n_steps=8, obs_dim=6, act_dim=7, device=torch.device("cpu"), close=lambda: None)
    with pytest.raises(NotImplementedError, match="attach_ppo_population: n_envs = 3 is not divisible by n_groups = 2"):
        env.attach_ppo_population(2)
    with pytest.raises(NotImplementedError, match=r"attach_ppo_population: batch_size = 32 does not divide m \* n_steps = 8"):
        env.attach_ppo_population(3, batch_size=32)
    assert env.ppo_population is None
    del env._device_path.buffers["rollout"]
    env.close()
    mixed = hrg.MixedHipVecEnv(NS(step_async=None, env_ids=["ReachHuman", "PickPlaceHumanCart"], slices=[slice(0, 2), slice(2, 4)]))
    with pytest.raises(NotImplementedError, match="attach_ppo_population: the mixed batch"):
        mixed.attach_ppo_population(2)


def test_the_header_declares_the_population_entries():
    from human_robot_gym_amd import _lib
    vp, i32, u64, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64, ctypes.c_double
    assert PROTOTYPES["hrg_ppo_population_create"] == (ctypes.c_int, [vp, i32, vp, i32, vp])
    assert PROTOTYPES["hrg_ppo_population_forward"] == (ctypes.c_int, [vp, vp, vp, i32, vp, i32, vp, vp, vp, vp])
    assert PROTOTYPES["hrg_ppo_population_export"] == (ctypes.c_int, [vp, i32] + [vp] * 5)
    assert {"hrg_ppo_population_create", "hrg_ppo_population_forward", "hrg_ppo_population_export"} <= set(_lib.EXPORTS)
    # the existing entries keep their signatures: a population's handle is an hrg_ppo, stepped, restored and destroyed by the lone learner's entries
    assert PROTOTYPES["hrg_ppo_create"] == (ctypes.c_int, [vp, i32, vp]) and PROTOTYPES["hrg_ppo_destroy"] == (None, [vp])
    assert PROTOTYPES["hrg_ppo_sizes"] == (ctypes.c_int, [vp, vp]) and PROTOTYPES["hrg_ppo_step"] == (ctypes.c_int, [vp] * 10 + [dbl, dbl, dbl, vp])
    assert PROTOTYPES["hrg_ppo_forward"] == (ctypes.c_int, [vp, vp, vp, i32, vp, i32, vp, vp, vp, vp]) and PROTOTYPES["hrg_ppo_export"] == (ctypes.c_int, [vp] * 6)
    assert PROTOTYPES["hrg_ppo_restore"] == (ctypes.c_int, [vp, u64, u64]) and PROTOTYPES["hrg_eval_policy_ppo"] == (ctypes.c_int, [vp] * 6)
    # no new entry on the buffers' handles: the grouped minibatch is the existing gather
    assert not [k for k in PROTOTYPES if "population" in k and k.startswith(("hrg_rollout_", "hrg_replay_"))]
    assert len(_lib.SOURCES) == 12


def test_grouped_minibatch_indices():
    """rollout.group_rows / group_table / group_batch on CPU tensors: P permutations of 0 .. m T - 1, group p's moved by p m T, a minibatch the groups' slices
    one behind the other."""
    n, T, P, B = 12, 8, 3, 16
    assert rollout.group_rows(n, T, P, B) == (3, 32) and rollout.group_rows(n, T, 1, 96) == (1, 96)
    with pytest.raises(NotImplementedError, match="n_envs = 12 is not divisible by n_groups = 5"):
        rollout.group_rows(n, T, 5, B)
    with pytest.raises(NotImplementedError, match=r"batch_size = 24 does not divide m \* n_steps = 32"):
        rollout.group_rows(n, T, P, 24)
    with pytest.raises(NotImplementedError, match="n_groups = 0"):
        rollout.group_rows(n, T, 0, B)
    rows = 32
    perms = [torch.randperm(rows, generator=torch.Generator().manual_seed(s)) for s in (4, 9, 4)]
    table = rollout.group_table(perms, rows)
    assert table.dtype == torch.int64 and tuple(table.shape) == (P, rows)
    seen = []
    for k0 in range(0, rows, B):
        idx = rollout.group_batch(table, k0, B)
        assert tuple(idx.shape) == (P * B,) and idx.is_contiguous()
        for p in range(P):
            mine = idx[p * B:(p + 1) * B]
            assert torch.equal(mine, perms[p][k0:k0 + B] + p * rows)   # the lone buffer's slice, moved into the group's range
            assert int(mine.min()) >= p * rows and int(mine.max()) < (p + 1) * rows
        seen.append(idx.reshape(P, B))
    epoch = torch.cat(seen, dim=1)
    for p in range(P):   # over one epoch a member's indices cover its range exactly once
        assert sorted(epoch[p].tolist()) == list(range(p * rows, (p + 1) * rows))
    assert torch.equal(table[0] + 2 * rows, table[2])   # the same seed draws the same permutation, whatever the group
    assert rollout.group_batch(rollout.group_table(perms[:1], rows), 16, 16).is_contiguous()   # one group: a view


def test_train_ppo_parses_seeds():
    spec = importlib.util.spec_from_file_location("train_ppo_tool", os.path.join(ROOT, "tools", "train_ppo.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)   # (imported: the parser only, nothing runs)
    args = tool.ap.parse_args(["--n-envs", "50", "--rollouts", "3", "--seeds", "0", "1", "2", "3", "4"])
    assert args.seeds == [0, 1, 2, 3, 4] and args.n_envs == 50 and args.seed == 0 and args.n_steps == 64 and args.batch_size == 64 and args.n_epochs == 20
    assert tool.ap.parse_args([]).seeds is None   # the default path: the lone learner
