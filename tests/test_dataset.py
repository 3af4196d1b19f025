"""Demonstration datasets, host side: the state-based imitation reward rules against the reference's recorded outputs (tests/golden/sir_ref.npz, written by
tools/make_sir_fixtures.py), the dataset file format, episode cutting, the config translation and the refusals.  No GPU."""
import ast
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest

import human_robot_gym_amd as hrg
import sir_ref as R
from human_robot_gym_amd import dataset as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sir_ref.npz")


@pytest.fixture(scope="module")
def fx():
    with np.load(GOLDEN) as z:
        d = {k: z[k] for k in z.files}
    d["params"] = ast.literal_eval(str(d["params"]))
    return d


def _ref_kwargs(kind, fn, p):
    """Arguments of sir_ref for the fixture's wrapper objects (pick-place: m_sim_fn is the name in the key, g_sim_fn the other one)."""
    if kind == "pick_place":
        return dict(beta=p["beta"], iota_m=p["iota_m"], iota_g=p["iota_g"], m_sim_fn=fn, g_sim_fn="tanh" if fn == "gaussian" else "gaussian")
    return dict(iota_m=p["iota"], m_sim_fn=fn)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("fn", ["gaussian", "tanh"])
def test_reward_and_early_termination_rules_match_the_reference(fx, kind, fn):
    """The same few FP64 operations as the wrappers: rewards to 1e-15 relative, verdicts exactly; every (gripped mismatch, verdict) group is populated."""
    p = fx["params"][kind]
    demo, pol = fx[kind + "_demo"], fx[kind + "_policy"]
    assert demo.shape == (321, 64) and demo.dtype == np.float32
    r_im, r_m, r_g, counted = R.imitation_reward(kind, demo, pol, **_ref_kwargs(kind, fn, p))
    want = fx[f"{kind}_{fn}_r_im"]
    rel = np.abs(r_im - want) / np.maximum(np.abs(want), 1e-300)
    print(f"[sir] {kind} {fn}: max relative difference of r_im {rel[want != 0].max() if (want != 0).any() else 0.0:.3e}; zero rewards {int((want == 0).sum())}")
    assert np.all(r_im[want == 0] == 0) and np.all(rel[want != 0] <= 1e-15)
    et = R.early_termination(kind, demo, pol, iota_m=p.get("iota", p.get("iota_m")), et_dist=p["et_dist"])
    np.testing.assert_array_equal(et, fx[f"{kind}_{fn}_et"])
    mm = R.mismatch(kind, demo, pol)
    if kind == "pick_place":   # the two terms the wrapper appends to its lists, and on which steps
        wm, wg = fx[f"{kind}_{fn}_r_motion"], fx[f"{kind}_{fn}_r_gripper"]
        np.testing.assert_array_equal(counted, ~np.isnan(wm))
        np.testing.assert_array_equal(counted, ~mm)
        assert np.all(np.abs(r_m[counted] - wm[counted]) <= 1e-15 * np.abs(wm[counted])) and np.all(np.abs(r_g[counted] - wg[counted]) <= 1e-15 * np.abs(wg[counted]))
    else:
        assert not counted.any() and np.all(np.isnan(fx[f"{kind}_{fn}_r_motion"]))
    assert np.all(r_im[mm] == 0)
    groups = [(False, False), (False, True)] + ([(True, True)] if kind != "reach" else []) + ([(True, False)] if kind == "pick_place" else [])
    for g in groups:
        assert ((mm == g[0]) & (et == g[1])).sum() >= 20, g
    assert R.et_margin(kind, demo, pol, iota_m=p.get("iota", p.get("iota_m")), et_dist=p["et_dist"]).min() >= 1e-9


def test_cursor_advances_and_saturates():
    np.testing.assert_array_equal(R.advance([0, 2, 3, 0], [1, 3, 3, 5]), [1, 3, 3, 1])


def _synthetic(env_id="PickPlaceHumanCart", lengths=(3, 1, 5), box=True, seed=0):
    rng = np.random.RandomState(seed)
    tt, n = int(sum(lengths)), len(lengths)
    return D.ExpertDataset(env_id, np.concatenate([[0], np.cumsum(lengths)]), rng.randint(0, 256, (tt, D.STATE_BYTES), dtype=np.uint8),
                           rng.uniform(-1, 1, (tt + n, 64)).astype(np.float32), rng.uniform(-1, 1, (tt, 7)),
                           boxes=rng.randint(0, 256, (tt, D.BOX_BYTES), dtype=np.uint8) if box else None, cartesian=box, obs_keys=["object_gripped", "vec_eef_to_object"],
                           ep_return=rng.uniform(-5, 0, n), ep_success=rng.rand(n) < 0.5)


def test_dataset_file_round_trips(tmp_path):
    ds = _synthetic()
    path = ds.save(str(tmp_path / "datasets" / "pp" / D.FILE_NAME))
    back = D.ExpertDataset.load(path, env_id="PickPlaceHumanCart", has_box=True)
    for k in ("ep_offset", "states", "boxes", "obs", "actions", "ep_return", "ep_success"):
        np.testing.assert_array_equal(getattr(back, k), getattr(ds, k), err_msg=k)
        assert getattr(back, k).dtype == getattr(ds, k).dtype
    assert (back.env_id, back.cartesian, back.robot_geometry, back.obs_keys, back.version) == (ds.env_id, True, "capsule", ds.obs_keys, D.library_version())
    assert (back.n_episodes, back.total_T, back.T(1), back.obs_row0(2)) == (3, 9, 1, 6)
    ep = back.episode(2)
    assert ep["states"].shape == (5, D.STATE_BYTES) and ep["obs"].shape == (6, 64) and np.array_equal(ep["obs"][-1], ds.obs[-1])
    nb = _synthetic("ReachHuman", box=False)
    assert D.ExpertDataset.load(nb.save(str(tmp_path / "r.npz")), env_id="ReachHuman", has_box=False).boxes is None
    # the restore copy: the recorded bytes with the time limit's step counter at zero, nothing else touched
    from human_robot_gym_amd._cstruct import EnvState
    rs, off = ds.restore_states(), EnvState.timestep.offset
    assert np.all(rs[:, off:off + 4] == 0) and np.array_equal(np.delete(rs, np.s_[off:off + 4], axis=1), np.delete(ds.states, np.s_[off:off + 4], axis=1))
    sub = ds.select([2, 0], lengths=[2, 3])
    assert sub.ep_offset.tolist() == [0, 2, 5] and np.array_equal(sub.obs[:3], ds.obs[6:9]) and np.array_equal(sub.states[2:], ds.states[:3])


def test_header_mismatches_are_refused(tmp_path):
    path = _synthetic().save(str(tmp_path / "d.npz"))
    with np.load(path) as z:
        good = {k: z[k] for k in z.files}

    def write(**over):
        p = str(tmp_path / "bad.npz")
        np.savez_compressed(p, **dict(good, **over))
        return p
    with pytest.raises(ValueError, match="hrg_state_bytes"):
        D.ExpertDataset.load(write(state_bytes=np.int64(D.STATE_BYTES + 8)))
    with pytest.raises(ValueError, match="hrg_state_bytes"):
        D.ExpertDataset.load(write(box_bytes=np.int64(8)))
    with pytest.raises(ValueError, match="recorded by"):
        D.ExpertDataset.load(write(version=np.array("hrgym-hip 0.0.9 (gfx950)")))
    with pytest.raises(ValueError, match="not of ReachHuman"):
        D.ExpertDataset.load(path, env_id="ReachHuman")
    with pytest.raises(ValueError, match="box"):
        D.ExpertDataset.load(path, env_id="PickPlaceHumanCart", has_box=False)
    with pytest.raises(ValueError, match="at least one transition"):   # an episode with T = 0
        D.ExpertDataset.load(write(ep_offset=np.array([0, 3, 3, 9])))
    with pytest.raises(ValueError, match="states of shape"):
        D.ExpertDataset.load(write(states=good["states"][:-1]))
    D.ExpertDataset.load(path)


def test_episode_cutting_on_a_synthetic_tape():
    """env 0: episodes of 3, 1 (a one-step episode) and 2 steps; env 1 never finishes; env 2: one episode that ends on the tape's last step."""
    done = np.zeros((6, 3), bool)
    done[[2, 3, 5], 0] = True
    done[5, 2] = True
    assert D.cut_episodes(done) == [(0, 0, 2), (0, 3, 3), (0, 4, 5), (2, 0, 5)]
    assert D.cut_episodes(done, 2) == [(0, 0, 2), (0, 3, 3)]      # the first n in (env, episode) order
    rng = np.random.RandomState(1)
    states, boxes = rng.randint(0, 256, (6, 3, D.STATE_BYTES), dtype=np.uint8), rng.randint(0, 256, (6, 3, D.BOX_BYTES), dtype=np.uint8)
    obs, term = rng.rand(6, 3, 64).astype(np.float32), rng.rand(6, 3, 64).astype(np.float32)
    act, rew, suc = rng.rand(6, 3, 7), rng.rand(6, 3).astype(np.float32), rng.rand(6, 3) < 0.5
    ds = D.assemble("PickPlaceHumanCart", D.cut_episodes(done), states, boxes, obs, term, act, rew, suc, cartesian=True)
    assert ds.ep_offset.tolist() == [0, 3, 4, 6, 12]
    e1 = ds.episode(1)   # the one-step episode: its state, its observation + the terminal one
    assert np.array_equal(e1["states"][0], states[3, 0]) and np.array_equal(e1["obs"], np.stack([obs[3, 0], term[3, 0]])) and np.array_equal(e1["actions"][0], act[3, 0])
    e3 = ds.episode(3)
    assert np.array_equal(e3["boxes"], boxes[:, 2]) and np.array_equal(e3["obs"][:-1], obs[:, 2]) and np.array_equal(e3["obs"][-1], term[5, 2])
    assert ds.ep_return[2] == pytest.approx(float(rew[4, 0]) + float(rew[5, 0])) and ds.ep_success.tolist() == [bool(suc[2, 0]), bool(suc[3, 0]), bool(suc[5, 0]), bool(suc[5, 2])]


def test_collector_refuses_a_tape_beyond_its_capacity_before_anything_is_allocated():
    assert D.tape_bytes(10, 4, True) == 10 * 4 * (D.STATE_BYTES + D.BOX_BYTES + 512 + 56 + 9)
    with pytest.raises(MemoryError, match="capacity_bytes"):   # 100 steps x 4096 envs x 4.4 KB: no batch is built (there is no GPU here)
        D.collect_expert_dataset("ReachHuman", 4096, 4096, expert=dict(id="ReachHuman"), capacity_bytes=1 << 30)
    with pytest.raises(NotImplementedError, match="further arrays"):
        D.collect_expert_dataset("CollaborativeStackingCart", 4, 4, expert=dict(id="PickPlaceHumanCart"))


def test_statistics_files(tmp_path):
    ds = _synthetic()
    D.write_stats(ds, str(tmp_path), [39, 40, 41, 42])
    rows = open(tmp_path / "observations.csv").read().splitlines()
    assert rows[0] == "mean,std" and len(rows) == 5
    v = ds.obs[:, 39:43].astype(np.float64)
    np.testing.assert_allclose([float(r.split(",")[0]) for r in rows[1:]], v.mean(axis=0), rtol=1e-15)
    np.testing.assert_allclose([float(r.split(",")[1]) for r in rows[1:]], v.std(axis=0), rtol=1e-15)
    head, vals = open(tmp_path / "stats.csv").read().splitlines()
    assert head == "success_mean,ep_len_mean,ep_len_std,ep_rew_mean,ep_rew_std"
    np.testing.assert_allclose([float(x) for x in vals.split(",")], [ds.ep_success.mean(), 3.0, np.std([3, 1, 5]), ds.ep_return.mean(), ds.ep_return.std()], rtol=1e-15)


def _config(**wrappers):
    cfg = NS(environment=NS(env_id="PickPlaceHumanCart", horizon=6), run=NS(), wrappers=NS(**wrappers))
    return cfg


SB = dict(alpha=0.5, beta=0.7, iota_m=0.1, iota_g=0.05, m_sim_fn="gaussian", g_sim_fn="tanh", observe_time=True, use_et=True, et_dist=2, verbose=False)
AB = dict(alpha=0.25, beta=0.7, iota_m=0.1, iota_g=0.5, m_sim_fn="gaussian", g_sim_fn="gaussian")
EXPERT = NS(id="PickPlaceHumanCart", signal_to_noise_ratio=0.98, obs_keys=["object_gripped"])


def test_config_translation_with_and_without_the_dataset_file(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    sb = _config(state_based_expert_imitation_reward=NS(dataset_name="pp-demo", rsi_prob=0.3, **SB))
    ab = _config(action_based_expert_imitation_reward=NS(dataset_name="pp-demo", rsi_prob=0.5, **AB))
    ab.expert = EXPERT
    with pytest.raises(NotImplementedError, match="state_based_expert_imitation_reward"):
        hrg.wrapper_kwargs_from_config(sb)
    with pytest.raises(NotImplementedError, match="DatasetRSIWrapper"):
        hrg.wrapper_kwargs_from_config(ab)
    with pytest.raises(NotImplementedError, match="state_based_expert_imitation_reward"):   # no dataset_name at all
        hrg.wrapper_kwargs_from_config(_config(state_based_expert_imitation_reward=NS(alpha=0.5)))
    _synthetic().save(D.dataset_path("pp-demo"))
    assert os.path.exists(tmp_path / "datasets" / "pp-demo" / "hrg_dataset.npz")
    kw = hrg.wrapper_kwargs_from_config(sb)
    assert kw == dict(dataset="pp-demo", rsi_prob=0.3, state_imitation_reward=SB)
    r = D.sir_kwargs("PickPlaceHumanCart", kw["state_imitation_reward"])
    assert r == dict(alpha=0.5, observe_time=True, use_et=True, et_dist=2.0, beta=0.7, iota_m=0.1, iota_g=0.05, m_sim_fn="gaussian", g_sim_fn="tanh")
    kw = hrg.wrapper_kwargs_from_config(ab)
    assert kw["dataset"] == "pp-demo" and kw["rsi_prob"] == 0.5 and kw["imitation_reward"] == AB and kw["expert"] == dict(id="PickPlaceHumanCart", signal_to_noise_ratio=0.98)
    with pytest.raises(NotImplementedError, match="DatasetRSIWrapper"):   # another name: still no file
        hrg.wrapper_kwargs_from_config(_config(action_based_expert_imitation_reward=NS(dataset_name="other", rsi_prob=0.5, **AB)))
    # ... and from there into the kernel argument
    ds = D.ExpertDataset.load("pp-demo", env_id="PickPlaceHumanCart", has_box=True)
    d, keep = D.build_dataset_desc(ds, rsi_prob=0.3, state_imitation_reward=SB, seed=7)
    assert (d.n_episodes, d.total_T, d.sir_kind, d.use_et, d.m_sim_fn, d.g_sim_fn, d.seed) == (3, 9, 2, 1, 0, 1, 7)
    assert (d.rsi_prob, d.alpha, d.beta, d.iota_m, d.iota_g, d.et_dist) == (0.3, 0.5, 0.7, 0.1, 0.05, 2.0)
    assert d.boxes == keep[2].ctypes.data and d.states == keep[1].ctypes.data and d.ep_offset == keep[0].ctypes.data and d.obs == keep[3].ctypes.data
    d, _ = D.build_dataset_desc(ds, rsi_prob=1.0)
    assert (d.sir_kind, d.rsi_prob, d.use_et) == (0, 1.0, 0)


def test_state_imitation_reward_arguments():
    r = D.sir_kwargs("ReachHuman", dict(alpha=0.3, iota=0.2, sim_fn="tanh", dataset_name="x", rsi_prob=0.5))
    assert (r["iota_m"], r["m_sim_fn"], r["beta"], r["observe_time"], r["use_et"], r["et_dist"]) == (0.2, "tanh", 1.0, True, False, 2.0)
    assert D.sir_kwargs("CollaborativeLiftingCart", dict(observe_time=False))["observe_time"] is False
    with pytest.raises(TypeError, match="iota_g"):
        D.sir_kwargs("ReachHuman", dict(iota_g=0.1))
    with pytest.raises(TypeError, match="sim_fn"):
        D.sir_kwargs("PickPlaceHumanCart", dict(sim_fn="tanh"))
    with pytest.raises(ValueError, match="Unknown similarity function"):
        D.sir_kwargs("PickPlaceHumanCart", dict(g_sim_fn="cosine"))
    with pytest.raises(NotImplementedError, match="HumanObjectInspectionCart"):
        D.sir_kwargs("HumanObjectInspectionCart", {})


def test_vec_env_refuses_what_it_cannot_run():
    from helpers import OracleBackend
    pp, ik = _synthetic(), dict(action_limit=0.1)
    with pytest.raises(NotImplementedError, match="backend"):
        hrg.HipVecEnv(2, env_id="PickPlaceHumanCart", backend=OracleBackend, dataset=pp, ik_position_delta=ik)
    with pytest.raises(NotImplementedError, match="goal_env"):
        hrg.HipVecEnv(2, env_id="PickPlaceHumanCart", goal_env=True, dataset=pp, ik_position_delta=ik)
    with pytest.raises(NotImplementedError, match="state based or action based"):
        hrg.HipVecEnv(2, env_id="PickPlaceHumanCart", dataset=pp, ik_position_delta=ik, expert=dict(id="PickPlaceHumanCart"), imitation_reward=dict(alpha=0.25),
                      state_imitation_reward=dict(alpha=0.5))
    for env_id in ("CollaborativeStackingCart", "CollaborativeHammeringCart"):
        with pytest.raises(NotImplementedError, match="further arrays"):
            hrg.HipVecEnv(2, env_id=env_id, dataset=pp)
    with pytest.raises(ValueError, match="need a dataset"):
        hrg.HipVecEnv(2, env_id="ReachHuman", rsi_prob=0.5)
    with pytest.raises(ValueError, match="need a dataset"):
        hrg.HipVecEnv(2, env_id="ReachHuman", state_imitation_reward=dict(alpha=0.5))
    with pytest.raises(ValueError, match="for ReachHuman"):   # a pick-place dataset (with its box array) for another task
        hrg.HipVecEnv(2, env_id="ReachHuman", dataset=pp)
    with pytest.raises(NotImplementedError, match="HumanObjectInspectionCart"):
        hrg.HipVecEnv(2, env_id="HumanObjectInspectionCart", dataset=_synthetic("HumanObjectInspectionCart"), state_imitation_reward=dict(alpha=0.5))
    for kw in (dict(dataset=pp), dict(rsi_prob=0.5), dict(state_imitation_reward=dict(alpha=0.5))):   # the mixed batch (refused before anything is built)
        with pytest.raises(NotImplementedError, match="per task"):
            hrg.make_mixed_vec_env(4, tasks=[("ReachHuman", {}), ("PickPlaceHumanCart", {})], **kw)


def test_abi_names_the_five_entry_points_and_the_header_stays_in_the_base_translation_unit():
    from human_robot_gym_amd import _lib
    from human_robot_gym_amd._cstruct import CONST, DatasetDesc
    for s in ("hrg_batch_snapshot", "hrg_batch_dataset_attach", "hrg_batch_dataset_reset", "hrg_batch_step_dataset", "hrg_batch_dataset_cursor"):
        assert s in _lib.EXPORTS
    assert (CONST["HRG_SIR_NONE"], CONST["HRG_SIR_REACH"], CONST["HRG_SIR_PICK_PLACE"], CONST["HRG_SIR_LIFTING"]) == (0, 1, 2, 3)
    assert CONST["HRG_SIR_DIM"] == 16 and [CONST["HRG_SIR_" + c.upper()] for c in D.SIR_COLUMNS] == list(range(14))
    assert {"n_episodes", "total_T", "ep_offset", "states", "boxes", "obs", "rsi_prob", "seed", "sir_kind", "alpha", "beta", "iota_m", "iota_g", "m_sim_fn", "g_sim_fn",
            "use_et", "et_dist"} == {f for f, _ in DatasetDesc._fields_}
    base = open(_lib.SRC).read()
    at = base.index('#include "hrgym_dataset.h"')
    assert base.rindex("#if HRG_BASE_TU", 0, at) > base.rindex("#endif", 0, at)   # inside the block that only the base translation unit compiles
    for src in _lib.SOURCES[1:]:
        assert "hrgym_dataset.h" not in open(src).read(), src
    assert any(os.path.basename(d) == "hrgym_dataset.h" for d in _lib.library_dependencies())
