"""Hyper-parameters per member of a population, the parts that need no handle: a scalar or one value per member, what stays shared, the table's
rows, the manifest of a population's folder, and --sweep of the training tools.  The device side: tests/test_sac_sweep_gpu.py, tests/test_ppo_sweep_gpu.py."""
import ctypes
import importlib.util
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tools_cases   # noqa: F401 (puts tools/ on the path, as for the golden cases)
from human_robot_gym_amd import _lib
from human_robot_gym_amd._cstruct import CONST, PROTOTYPES, PpoHyper, SacHyper
from human_robot_gym_amd._learner import (MANIFEST, MAX_POPULATION, check_members, load_checkpoint, per_member, read_manifest, refuse_shared_sequences, save_checkpoint,
                                          write_manifest)
from human_robot_gym_amd.ppo import PpoLearner, PpoPopulation, build_ppo_desc
from human_robot_gym_amd.sac import SacLearner, SacPopulation, build_sac_desc, parse_ent_coef
from human_robot_gym_amd.training_utils import member_lines, sweep_members

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_scalar_means_every_member_and_a_sequence_one_value_each():
    assert per_member("gamma", 0.9, 3) == [0.9, 0.9, 0.9]
    assert per_member("ent_coef", "auto_0.2", 2) == ["auto_0.2", "auto_0.2"] and per_member("clip_range_vf", None, 2) == [None, None]   # a string and None are scalars
    assert per_member("tau", (0.1, 0.2), 2) == [0.1, 0.2] and per_member("tau", np.array([0.1, 0.2]), 2) == [0.1, 0.2]
    for bad in ([0.1, 0.2], [0.1] * 4, []):
        with pytest.raises(ValueError, match=f"learning_rate: {len(bad)} values for 3 members"):
            per_member("learning_rate", bad, 3)
    assert SacPopulation.member_values(3, learning_rate=1e-3, gamma=[0.99, 0.9, 0.95]) == dict(learning_rate=[1e-3] * 3, gamma=[0.99, 0.9, 0.95])
    with pytest.raises(ValueError, match="tau: 2 values for 3 members"):
        SacPopulation.member_values(3, tau=[0.1, 0.2])
    with pytest.raises(ValueError, match="clip_range: 4 values for 3 members"):
        PpoPopulation.member_values(3, clip_range=[0.1] * 4)


def test_the_tables_fields_are_the_headers_rows():
    assert [n for n, _ in SacHyper._fields_ if not n.endswith("_")] == ["learning_rate", "gamma", "tau", "ent_coef", "target_entropy", "auto_ent_coef"]
    assert [n for n, _ in PpoHyper._fields_] == list(PpoPopulation._fields) == ["learning_rate", "clip_range", "clip_range_vf", "ent_coef", "vf_coef", "max_grad_norm"]
    assert SacPopulation._fields == ("learning_rate", "gamma", "tau", "ent_coef", "target_entropy")
    assert ctypes.sizeof(SacHyper) == 48 and ctypes.sizeof(PpoHyper) == 48
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    for prefix in ("hrg_sac", "hrg_ppo"):
        assert PROTOTYPES[prefix + "_population_set_hyper"] == (ctypes.c_int, [vp, vp, i32, vp]) and prefix + "_population_set_hyper" in _lib.EXPORTS
    # the entries that were there keep their signatures
    assert PROTOTYPES["hrg_sac_step"][1] == [vp] * 12 + [ctypes.c_double, vp] and PROTOTYPES["hrg_ppo_step"][1] == [vp] * 10 + [ctypes.c_double] * 3 + [vp]
    assert MAX_POPULATION == CONST["HRG_SAC_MAX_POPULATION"] == 64


def test_what_shapes_a_launch_or_the_lockstep_is_shared():
    for name, value in (("batch_size", [32, 64]), ("net_arch", [[64], [64, 64]]), ("target_update_interval", (1, 2))):
        with pytest.raises(NotImplementedError, match=f"{name} = .*one value per member is not supported: "):
            refuse_shared_sequences(SacPopulation._shared, {name: value})
    for name, value in (("batch_size", [32, 64]), ("net_arch", [[64], [64, 64]]), ("net_arch", [[dict(pi=[64], vf=[64])], [64]]), ("n_epochs", [2, 3]),
                        ("normalize_advantage", [True, False]), ("rollout_size", [64, 128])):
        with pytest.raises(NotImplementedError, match=f"{name} = .*one value per member is not supported: "):
            refuse_shared_sequences(PpoPopulation._shared, {name: value})
    # a net_arch is a list by itself, and scalars pass
    refuse_shared_sequences(SacPopulation._shared, dict(net_arch=[64, 64, 64], batch_size=128, target_update_interval=1))
    refuse_shared_sequences(PpoPopulation._shared, dict(net_arch=[dict(pi=[64, 64], vf=[64, 64])], batch_size=64, n_epochs=20, learning_rate=[1e-3, 1e-4]))
    assert not set(SacPopulation._shared) & set(SacPopulation._fields) and not set(PpoPopulation._shared) & set(PpoPopulation._fields)
    # the constructors refuse before they look for a device
    with pytest.raises(NotImplementedError, match="batch_size = .*the batch shapes every launch"):
        SacPopulation(6, 4, 2, (0, 1), batch_size=[32, 64])
    with pytest.raises(NotImplementedError, match="n_epochs = .*the host's loop"):
        PpoPopulation(6, 4, 2, (0, 1), n_epochs=[2, 3])


def test_ent_coef_per_member_mixes_learned_and_fixed():
    values = SacPopulation.member_values(3, ent_coef=["auto", "auto_0.2", 0.1], target_entropy=["auto", "auto", -2.0])
    assert values == dict(ent_coef=["auto", "auto_0.2", 0.1], target_entropy=["auto", "auto", -2.0])
    assert [parse_ent_coef(v) for v in values["ent_coef"]] == [(True, 1.0), (True, 0.2), (False, 0.1)]
    descs = [build_sac_desc(6, 4, ent_coef=e, target_entropy=t, batch_size=32) for e, t in zip(values["ent_coef"], values["target_entropy"])]
    assert [(d.auto_ent_coef, d.ent_coef, d.target_entropy) for d in descs] == [(1, 1.0, -4.0), (1, 0.2, -4.0), (0, 0.1, -2.0)]
    for bad, match in ((["auto", "fixed"], "ent_coef = 'fixed'"), ([0.1, -0.1], "positive"), (["auto_0", 0.1], "greater than 0")):
        with pytest.raises(ValueError, match=match):
            SacPopulation.member_values(2, ent_coef=bad)
    for name, bad in (("gamma", [0.9, 1.5]), ("tau", [-0.1, 0.5]), ("learning_rate", [1e-3, -1e-3]), ("gamma", [0.9, float("nan")])):
        with pytest.raises(ValueError, match=name):
            SacPopulation.member_values(2, **{name: bad})


def test_clip_range_vf_none_is_the_negative_sentinel_and_back(tmp_path):
    values = PpoPopulation.member_values(2, clip_range_vf=[None, 0.3], **{k: v for k, v in PpoPopulation._defaults.items() if k != "clip_range_vf"})
    assert values["clip_range_vf"] == [None, 0.3] and values["clip_range"] == [0.2, 0.2]
    rows = [PpoPopulation.table_row({k: v[p] for k, v in values.items()}) for p in range(2)]
    assert [r.clip_range_vf for r in rows] == [-1.0, 0.3] and [r.max_grad_norm for r in rows] == [0.5, 0.5] and [r.vf_coef for r in rows] == [0.5, 0.5]
    # ... and back: a checkpoint stores None as NaN, and the constructor's keyword is None again
    for p, vf in enumerate(values["clip_range_vf"]):
        path = save_checkpoint(str(tmp_path / f"member_{p}.npz"), "hrg_ppo", build_ppo_desc(6, 4, net_arch=[64], batch_size=32), _tensors(10),
                               (0, 0), dict(learning_rate=3e-4, clip_range=0.2, clip_range_vf=vf, n_epochs=10))
        ckpt = load_checkpoint(path, "hrg_ppo")
        assert math.isnan(float(ckpt["hyper"]["clip_range_vf"])) == (vf is None) and PpoLearner._checkpoint_kwargs(ckpt["desc"], ckpt["hyper"])["clip_range_vf"] == vf
    for name, bad in (("clip_range_vf", [None, 0.0]), ("clip_range", [0.2, 0.0]), ("max_grad_norm", [0.5, -1.0]), ("ent_coef", [0.0, -0.01]), ("vf_coef", [0.5, float("inf")])):
        with pytest.raises(ValueError, match=name):
            PpoPopulation.member_values(2, **{name: bad})


# ---- the manifest, on hand-made checkpoints ----
def _tensors(n, target=False):
    p = SimpleNamespace(params=torch.zeros(n), adam_m=torch.zeros(n), adam_v=torch.zeros(n))
    if target:
        p.target = torch.zeros(4)
    return p


def _sac_folder(folder, members, varies=None):
    """member_<p>.npz of hand-made SAC checkpoints, one per dict of (learning_rate, descriptor keywords), and the manifest where `varies` is given."""
    os.makedirs(folder, exist_ok=True)
    for p, kw in enumerate(members):
        kw = dict(kw)
        lr = kw.pop("learning_rate", 3e-4)
        save_checkpoint(os.path.join(folder, f"member_{p}.npz"), "hrg_sac", build_sac_desc(6, 4, batch_size=32, seed=p, **kw), _tensors(10, target=True), (3, 1),
                        dict(learning_rate=lr))
    if varies is not None:
        write_manifest(folder, "hrg_sac", varies)
    files = [os.path.join(folder, f"member_{p}.npz") for p in range(len(members))]
    return files, [load_checkpoint(f, "hrg_sac") for f in files]


def test_a_manifest_lets_the_fields_it_names_differ_and_nothing_else(tmp_path):
    may = SacPopulation._manifest_fields
    folder = str(tmp_path / "lr")
    files, ckpts = _sac_folder(folder, [dict(learning_rate=1e-3), dict(learning_rate=3e-4)], varies=["learning_rate"])
    assert read_manifest(folder, "hrg_sac") == ("learning_rate",)
    check_members(files, ckpts, read_manifest(folder, "hrg_sac"), may)   # learning_rate may differ ...
    files, ckpts = _sac_folder(str(tmp_path / "lr_gamma"), [dict(learning_rate=1e-3), dict(learning_rate=3e-4, gamma=0.9)], varies=["learning_rate"])
    with pytest.raises(ValueError, match="member_1.npz: gamma differ from member 0's: the members of a population share them"):   # ... and nothing else
        check_members(files, ckpts, ("learning_rate",), may)
    files, ckpts = _sac_folder(str(tmp_path / "ent"), [dict(ent_coef="auto_0.2"), dict(ent_coef=0.1)], varies=["ent_coef", "auto_ent_coef"])
    check_members(files, ckpts, ("auto_ent_coef", "ent_coef"), may)
    with pytest.raises(ValueError, match="member_1.npz: auto_ent_coef differ"):
        check_members(files, ckpts, ("ent_coef",), may)
    # a manifest cannot name what the members share, nor excuse other counters
    files, ckpts = _sac_folder(str(tmp_path / "shape"), [dict(), dict()])
    with pytest.raises(ValueError, match="the manifest names batch_size: the members of a population share them"):
        check_members(files, ckpts, ("batch_size",), may)
    ckpts[1]["counters"] = np.array([4, 1], np.uint64)
    with pytest.raises(ValueError, match="member_1.npz: counters differ"):
        check_members(files, ckpts, may, may)


def test_without_a_manifest_the_old_rule_and_its_words_hold(tmp_path):
    folder = str(tmp_path / "none")
    files, ckpts = _sac_folder(folder, [dict(learning_rate=1e-3), dict(learning_rate=3e-4)])
    assert read_manifest(folder, "hrg_sac") == () and not os.path.exists(os.path.join(folder, MANIFEST))
    with pytest.raises(ValueError, match="member_1.npz: learning_rate differ from member 0's: the members of a population share them"):
        check_members(files, ckpts, read_manifest(folder, "hrg_sac"), SacPopulation._manifest_fields)
    with pytest.raises(ValueError, match="member_1.npz: learning_rate differ from member 0's: the members of a population share them"):
        SacPopulation.load(folder)   # (refused before a device is looked for)
    files, ckpts = _sac_folder(str(tmp_path / "same"), [dict(), dict()])
    check_members(files, ckpts)


def test_the_manifest_holds_arrays_only(tmp_path):
    folder = str(tmp_path)
    path = write_manifest(folder, "hrg_ppo", ["learning_rate", "clip_range_vf"])
    assert path == os.path.join(folder, MANIFEST)
    with np.load(path, allow_pickle=False) as f:   # no pickled data: this load refuses object arrays
        arrays = {k: f[k] for k in f.files}
    assert sorted(arrays) == ["format", "kind", "varies"] and all(a.dtype != object for a in arrays.values())
    assert list(arrays["varies"]) == ["clip_range_vf", "learning_rate"] and str(arrays["kind"]) == "hrg_ppo"
    assert read_manifest(folder, "hrg_ppo") == ("clip_range_vf", "learning_rate")
    with pytest.raises(ValueError, match="no manifest of a population of 'hrg_sac'"):
        read_manifest(folder, "hrg_sac")
    assert write_manifest(folder, "hrg_ppo", []) is None and not os.path.exists(path)   # nothing varies: no manifest, and a stale one goes


# ---- --sweep of the training tools ----
def _tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)   # (imported: the parser and members_of only, nothing runs)
    return tool


def test_train_sac_crosses_sweeps_with_each_other_and_with_the_seeds():
    tool = _tool("train_sac")
    base = ["--gradient-steps", "8"]
    args = tool.ap.parse_args(base + ["--n-envs", "24", "--seeds", "0", "1", "2", "--sweep", "learning_rate=1e-3,3e-4", "--sweep", "ent_coef=auto_0.2,0.1"])
    seeds, swept = tool.members_of(args)
    assert seeds == [0, 1, 2] * 4                                                      # seed-minor
    assert swept["learning_rate"] == [1e-3] * 6 + [3e-4] * 6                            # value-major: the first sweep changes slowest
    assert swept["ent_coef"] == (["auto_0.2"] * 3 + [0.1] * 3) * 2 and list(swept) == ["learning_rate", "ent_coef"]
    args = tool.ap.parse_args(base + ["--n-envs", "8", "--seed", "5", "--sweep", "tau=0.005,0.05"])   # without --seeds: --seed alone
    assert tool.members_of(args) == ([5, 5], dict(tau=[0.005, 0.05]))
    assert tool.ap.parse_args(base).sweep is None and tool.ap.parse_args(base + ["--sweep", "target-entropy=-2,-4", "--n-envs", "2"]).sweep == ["target-entropy=-2,-4"]
    assert tool.members_of(tool.ap.parse_args(base + ["--sweep", "target-entropy=-2,-4", "--n-envs", "2"]))[1] == dict(target_entropy=[-2.0, -4.0])
    for extra, match in ((["--sweep", "batch_size=64,128"], "batch_size is no per-member field"), (["--sweep", "clip_range=0.1,0.2"], "clip_range is no per-member field"),
                         (["--sweep", "gamma"], "expected NAME=v1,v2"), (["--sweep", "gamma=0.9,,0.8"], "expected NAME=v1,v2"),
                         (["--sweep", "gamma=0.9,0.8", "--sweep", "gamma=0.7"], "gamma is swept twice"),
                         (["--n-envs", "25", "--seeds", "0", "1", "2", "--sweep", "gamma=0.9,0.8"], "--n-envs 25 is not divisible by the 6 members"),
                         (["--n-envs", "1300", "--seeds", *map(str, range(13)), "--sweep", "gamma=0.9,0.8,0.7,0.6,0.5"], f"13 = 65 members: a population has 1 .. {MAX_POPULATION}")):
        with pytest.raises(ValueError, match=match):
            tool.members_of(tool.ap.parse_args(base + extra))


def test_train_ppo_crosses_sweeps_with_each_other_and_with_the_seeds():
    tool = _tool("train_ppo")
    args = tool.ap.parse_args(["--n-envs", "60", "--seeds", "3", "4", "--sweep", "clip_range=0.1,0.2,0.3", "--sweep", "clip_range_vf=none,0.3"])
    seeds, swept = tool.members_of(args)
    assert seeds == [3, 4] * 6 and swept["clip_range"] == [0.1] * 4 + [0.2] * 4 + [0.3] * 4 and swept["clip_range_vf"] == ([None] * 2 + [0.3] * 2) * 3
    assert tool.members_of(tool.ap.parse_args(["--n-envs", "4", "--sweep", "ent_coef=0,0.01"])) == ([0, 0], dict(ent_coef=[0.0, 0.01]))
    for extra, match in ((["--sweep", "n_epochs=2,3"], "n_epochs is no per-member field"), (["--sweep", "gamma=0.9,0.8"], "gamma is no per-member field"),
                         (["--n-envs", "50", "--sweep", "vf_coef=0.5,0.25,1"], "--n-envs 50 is not divisible by the 3 members"),
                         (["--n-envs", "650", "--seeds", *map(str, range(5)), "--sweep", "max_grad_norm=" + ",".join(str(0.1 * k) for k in range(1, 14))],
                          "13 x 5 = 65 members")):
        with pytest.raises(ValueError, match=match):
            tool.members_of(tool.ap.parse_args(extra))
    assert sweep_members(None, [0, 1], 4, PpoPopulation._fields, MAX_POPULATION) == ([0, 1], {})   # --seeds alone: the population of before


def test_a_members_swept_values_stand_beside_diagnostics_of_the_same_name():
    """The diagnostics report learning_rate, clip_range, clip_range_vf (PPO) and the live ent_coef (SAC) under the swept fields' own names: the members' lines
    keep the swept values under `hyper`, whatever overlaps."""
    stats = [dict(episodes=2, r=1.0, l=10), dict(episodes=3, r=2.0, l=20)]
    diag = [dict(loss=0.5, clip_range=0.1, learning_rate=1e-3, clip_range_vf=0.3, n_updates=4), dict(loss=0.25, clip_range=0.2, learning_rate=1e-3, n_updates=4)]
    swept = dict(clip_range=[0.1, 0.2], clip_range_vf=[0.3, None], learning_rate=[1e-3, 1e-3])
    lines = member_lines([7, 8], swept, stats, diag)
    assert lines[0] == dict(seed=7, hyper=dict(clip_range=0.1, clip_range_vf=0.3, learning_rate=1e-3), episodes=2, r=1.0, l=10, **diag[0])
    assert lines[1]["hyper"] == dict(clip_range=0.2, clip_range_vf=None, learning_rate=1e-3) and lines[1]["clip_range"] == 0.2 and "clip_range_vf" not in lines[1]
    sac = member_lines([0, 1], dict(ent_coef=["auto_0.2", 0.1]), stats, [dict(ent_coef=0.1873, actor_loss=1.0), dict(ent_coef=0.1, actor_loss=2.0)])
    assert [m["hyper"]["ent_coef"] for m in sac] == ["auto_0.2", 0.1] and [m["ent_coef"] for m in sac] == [0.1873, 0.1]   # the swept value and the live one
    assert member_lines([0, 1], dict(ent_coef=["auto_0.2", 0.1]), stats)[1] == dict(seed=1, hyper=dict(ent_coef=0.1), **stats[1])   # before the first update
    assert member_lines([3, 4], {}, stats, diag)[0] == dict(seed=3, **stats[0], **diag[0])   # --seeds alone: the lines of before
    json.dumps(lines), json.dumps(sac)


def test_swept_values_no_learner_takes_are_refused_before_any_env_is_built():
    sac, ppo = _tool("train_sac"), _tool("train_ppo")
    for extra, match in ((["--sweep", "gamma=0.9,nan"], "gamma"), (["--sweep", "learning_rate=1e-3,-1"], "learning_rate"), (["--sweep", "tau=0.1,1.5"], "tau"),
                         (["--sweep", "ent_coef=auto_0.2,fixed"], "ent_coef"), (["--sweep", "ent_coef=0.1,-0.1"], "positive")):
        with pytest.raises(ValueError, match=match):
            sac.members_of(sac.ap.parse_args(["--gradient-steps", "8", "--n-envs", "8"] + extra))
    for extra, match in ((["--sweep", "clip_range=0.1,0"], "clip_range"), (["--sweep", "clip_range_vf=none,-0.3"], "clip_range_vf"), (["--sweep", "vf_coef=0.5,inf"], "vf_coef"),
                         (["--sweep", "max_grad_norm=0.5,auto"], "could not convert")):
        with pytest.raises(ValueError, match=match):
            ppo.members_of(ppo.ap.parse_args(["--n-envs", "8"] + extra))


def test_the_lone_learners_read_their_scalars_as_before():
    assert SacLearner._scalar(SimpleNamespace(learning_rate=1e-3), "learning_rate") == 1e-3
    assert PpoLearner._scalar(SimpleNamespace(clip_range_vf=None), "clip_range_vf", member=0) is None
