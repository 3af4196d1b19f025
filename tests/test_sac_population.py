"""The SAC population, host side: the seeds table and the stacked tensors, the refusals that come before the device is touched, the ABI and the tool's
parser.  No GPU.  What a member computes is tests/test_sac_population_gpu.py's."""
import ctypes
import importlib.util
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import human_robot_gym_amd as hrg
from helpers import OracleBackend
from human_robot_gym_amd import sac
from human_robot_gym_amd._cstruct import CONST, PROTOTYPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_seeds_table_and_descriptor():
    assert CONST["HRG_SAC_MAX_POPULATION"] == sac.MAX_POPULATION == 64
    P, table = sac.check_seeds(3, (5, 9, -1))
    assert P == 3 and table.dtype == np.uint64 and table.tolist() == [5, 9, 2**64 - 1]   # (a seed is its low 64 bits, as build_sac_desc keeps it)
    assert sac.check_seeds(1, [7])[1].tolist() == [7] and sac.check_seeds(64, range(64))[0] == 64
    d = sac.build_sac_desc(6, 4, batch_size=64, seed=9)
    assert ctypes.sizeof(d) == 32 + 4 * 8 + 8   # the descriptor a population shares is the lone learner's, unchanged


@pytest.mark.parametrize("P", [0, 65, -1])
def test_members_outside_the_range_are_refused(P):
    with pytest.raises(NotImplementedError, match=f"n_members = {P}"):
        sac.check_seeds(P, range(max(P, 0)))
    with pytest.raises(NotImplementedError, match=f"n_members = {P}"):   # before the device or the library is touched
        sac.SacPopulation(6, 4, P, list(range(max(P, 0))), batch_size=64)


def test_wrong_number_of_seeds_and_whatever_the_lone_learner_refuses():
    with pytest.raises(ValueError, match="2 seeds for 3 members"):
        sac.SacPopulation(6, 4, 3, [1, 2], batch_size=64)
    with pytest.raises(NotImplementedError, match="batch_size = 48"):
        sac.SacPopulation(6, 4, 2, [1, 2], batch_size=48)
    with pytest.raises(NotImplementedError, match="net_arch"):
        sac.SacPopulation(6, 4, 2, [1, 2], net_arch=[32], batch_size=64)


def test_parameter_rows_are_the_lone_learners_initialisation():
    seeds = (5, 9, 2)
    pop = sac.SacPopulationParams(6, 4, 2, seeds, ent_coef_init=0.2)
    n, n_actor, n_critic = sac.param_layout(6, 4, 2)[1]
    assert tuple(pop.params.shape) == tuple(pop.adam_m.shape) == tuple(pop.adam_v.shape) == (3, n) and tuple(pop.target.shape) == (3, 2 * n_critic)
    assert (pop.n_params, pop.n_actor, pop.n_critic) == (n, n_actor, n_critic)
    for p, s in enumerate(seeds):
        lone = sac.SacParams(6, 4, 2, seed=s, ent_coef_init=0.2)
        assert torch.equal(pop.params[p], lone.params) and torch.equal(pop.target[p], lone.target)
        assert not pop.adam_m[p].any() and not pop.adam_v[p].any()
        m = pop.member(p)
        assert m.params.data_ptr() == pop.params[p].data_ptr() and m.target.is_contiguous()   # views: a checkpoint restored into them lands in the rows
    assert not torch.equal(pop.params[0], pop.params[1])
    assert float(pop.params[2, -1]) == pytest.approx(np.log(0.2))


def _oracle_env(n, **kw):
    clips = hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300)
    ek = dict(shield_type="OFF", horizon=5)
    return hrg.HipVecEnv(n, env_kwargs=ek, clips=clips, backend=OracleBackend(hrg.build_model_desc(ek, n_clips=2), clips, n), **kw)


def test_attach_refusals_by_name():
    env = _oracle_env(3)
    assert env.sac_population is None
    with pytest.raises(NotImplementedError, match="num_envs = 3 is not divisible by n_members = 2"):
        env.attach_sac_population(2)
    with pytest.raises(NotImplementedError, match="n_members = 65"):
        env.attach_sac_population(65)
    with pytest.raises(ValueError, match="1 seeds for 3 members"):
        env.attach_sac_population(3, seeds=[4])
    with pytest.raises(TypeError, match="seeds"):
        env.attach_sac_population(3, seed=4)
    with pytest.raises(NotImplementedError, match="attach_sac_population: the replay kernels run in the HIP library"):   # (another backend has no buffer to read)
        env.attach_sac_population(3)
    assert env.sac_population is None
    env.close()
    goal = _oracle_env(2, goal_env=True)
    with pytest.raises(NotImplementedError, match="attach_sac_population: goal_env: the hindsight buffer has no grouped sample"):
        goal.attach_sac_population(2)
    goal.close()
    mixed = hrg.MixedHipVecEnv(NS(step_async=None, env_ids=["ReachHuman", "PickPlaceHumanCart"], slices=[slice(0, 2), slice(2, 4)]))
    with pytest.raises(NotImplementedError, match="attach_sac_population: the mixed batch"):
        mixed.attach_sac_population(2)


def test_the_header_declares_the_population_entries():
    from human_robot_gym_amd import _lib
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    assert PROTOTYPES["hrg_sac_population_create"] == (ctypes.c_int, [vp, i32, vp, i32, vp])
    assert PROTOTYPES["hrg_sac_population_act"] == (ctypes.c_int, [vp, vp, vp, i32, vp, i32, vp, vp])
    assert PROTOTYPES["hrg_sac_population_export"] == (ctypes.c_int, [vp, i32] + [vp] * 6)
    assert PROTOTYPES["hrg_sac_population_sample"] == (ctypes.c_int, [vp, i32, i32] + [vp] * 8)
    assert {k for k in PROTOTYPES if "population" in k} <= set(_lib.EXPORTS)
    # the existing entries keep their signatures: a population's handle is an hrg_sac, stepped, restored and destroyed by the lone learner's entries
    assert PROTOTYPES["hrg_sac_create"] == (ctypes.c_int, [vp, i32, vp]) and PROTOTYPES["hrg_sac_step"][1] == [vp] * 12 + [ctypes.c_double, vp]
    assert PROTOTYPES["hrg_sac_act"][1] == [vp, vp, vp, i32, vp, i32, vp, vp] and PROTOTYPES["hrg_replay_sample"] == (ctypes.c_int, [vp, i32] + [vp] * 8)
    assert len(_lib.SOURCES) == 12


def test_train_sac_parses_seeds():
    spec = importlib.util.spec_from_file_location("train_sac_tool", os.path.join(ROOT, "tools", "train_sac.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)   # (imported: the parser only, nothing runs)
    args = tool.ap.parse_args(["--gradient-steps", "800", "--n-envs", "1280", "--seeds", "0", "1", "2", "3", "4"])
    assert args.seeds == [0, 1, 2, 3, 4] and args.n_envs == 1280 and args.seed == 0
    assert tool.ap.parse_args(["--gradient-steps", "8"]).seeds is None   # the default path: the lone learner
