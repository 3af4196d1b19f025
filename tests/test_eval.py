"""Evaluation, the parts that need no GPU: tests/eval_ref.py against a literal transcription of SB3's loop and its own invariants, the descriptor's refusals,
the checkpoint round trip on CPU tensors, the reference's checkpoint names, the config translation, the ABI's entries."""
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest

import eval_ref as E
import replay_ref as R
from human_robot_gym_amd import _learner as L
from human_robot_gym_amd import evaluation as EV
from human_robot_gym_amd import training_utils as TU
from human_robot_gym_amd._cstruct import CONST, PROTOTYPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference", "training", "config_icra_2024", "environment_evaluation", "training")
CASES = [(6, 1, 8), (6, 3, 5), (4, 2, 3), (5, 1, 1)]   # n_envs, n_policies, n_eval_episodes


def _run(n, P, N, steps=12, seed=0, rows=None):
    """A ledger fed `steps` scripted steps (replay_ref.scripted_steps with eval_ref.done_pattern); returns (ledger, the steps)."""
    led, fed = E.Ledger(n, P, N), []
    for st in R.scripted_steps(n, steps, 7, seed, done=E.done_pattern(n, steps, seed)):
        _, _, _, rew, dn, info, imit, sir = st
        led.step(rew, dn, info, **({} if rows is None else dict(imit=imit) if rows == "imit" else dict(sir=sir)))
        fed.append(st)
    return led, fed


@pytest.mark.parametrize("n,P,N", CASES)
def test_quotas_sum_to_the_episodes_asked_for_and_are_met(n, P, N):
    led, _ = _run(n, P, N)
    m = n // P
    t = led.targets.reshape(P, m)
    assert (t.sum(axis=1) == N).all() and t.max() - t.min() <= 1 and (np.diff(t, axis=1) >= 0).all()   # also for N not a multiple of m
    np.testing.assert_array_equal(EV.quotas(n, P, N), led.targets)
    assert led.remaining() == 0 and (led.counts == led.targets).all()   # the done patterns meet every quota within the scripted steps
    assert [len(led.episode_rewards(k)) for k in range(P)] == [N] * P and len(led.episodes) == N * P


def test_the_restatement_is_sb3s_loop():
    """One group: a literal transcription of evaluate_policy's loop over Monitor-style infos gives the same lists."""
    n, N, steps = 6, 8, 12
    led, fed = _run(n, 1, N, steps)
    episode_rewards, episode_lengths, counts = [], [], np.zeros(n, int)
    count_targets = np.array([(N + i) // n for i in range(n)], dtype="int")
    mon_r, mon_l = [[] for _ in range(n)], np.zeros(n, int)
    for _, _, _, rew, dn, info, _, _ in fed:
        if not (counts < count_targets).any():
            break
        infos = [{} for _ in range(n)]
        for i in range(n):   # Monitor.step
            mon_r[i].append(float(rew[i]))
            mon_l[i] += 1
            if dn[i]:
                infos[i]["episode"] = {"r": sum(mon_r[i]), "l": int(mon_l[i])}
                mon_r[i], mon_l[i] = [], 0
        for i in range(n):
            if counts[i] < count_targets[i] and dn[i] and "episode" in infos[i]:
                episode_rewards.append(infos[i]["episode"]["r"])
                episode_lengths.append(infos[i]["episode"]["l"])
                counts[i] += 1
    assert led.episode_rewards() == episode_rewards and led.episode_lengths() == episode_lengths and len(episode_rewards) == N


def test_steps_behind_the_quota_are_ignored_and_the_order_is_by_step_then_env():
    led, fed = _run(6, 3, 5, steps=12)
    before = [dict(e) for e in led.episodes]
    for st in R.scripted_steps(6, 5, 7, 99, done=np.ones((5, 6), np.uint8)):   # every quota is met: nothing more is appended
        led.step(st[3], st[4], st[5])
    assert len(led.episodes) == len(before) and led.remaining() == 0
    key = [(e["step"], e["env"]) for e in led.episodes]
    assert key == sorted(key) and len(set(key)) == len(key)
    # an episode's return covers the steps since the env's previous done -- counted or not -- and the info row is the done step's
    for e in led.episodes:
        t0 = e["step"] - e["l"] + 1
        assert t0 == 0 or fed[t0 - 1][4][e["env"]]
        assert all(not fed[t][4][e["env"]] for t in range(t0, e["step"])) and fed[e["step"]][4][e["env"]]
        assert e["r"] == float(sum(np.float64(fed[t][3][e["env"]]) for t in range(t0, e["step"] + 1)))
        np.testing.assert_array_equal(e["info"], fed[e["step"]][5][e["env"]])


def test_monitors_return_is_the_envs_own_reward_under_an_imitation_reward():
    plain, fed = _run(6, 1, 8)
    for rows, col in (("imit", E.IMIT_R_ENV), ("sir", E.SIR_R_ENV)):
        led, _ = _run(6, 1, 8, rows=rows)
        assert [(e["env"], e["step"], e["l"]) for e in led.episodes] == [(e["env"], e["step"], e["l"]) for e in plain.episodes]
        src = 6 if rows == "imit" else 7
        for e in led.episodes:
            assert e["r"] == float(sum(np.float64(fed[t][src][e["env"], col]) for t in range(e["step"] - e["l"] + 1, e["step"] + 1))) != 0
            assert e["ep_im"] == float(fed[e["step"]][src][e["env"], E.IMIT_EP_IM if rows == "imit" else E.SIR_EP_IM])
        assert led.episode_rewards() != plain.episode_rewards()


def test_records_and_the_result_built_from_them_keep_the_order_and_the_split():
    led, _ = _run(6, 3, 5)
    counts, rec = led.records(3)
    assert rec.shape == (6, 3, CONST["HRG_EVAL_RECORD_DIM"]) == (6, 3, E.RECORD_DIM) and (counts == led.targets).all()
    assert [CONST["HRG_EVAL_REC_" + k] for k in ("RETURN", "LENGTH", "STEP", "TRUNCATED", "INFO", "EP_IM")] == [E.REC_RETURN, E.REC_LENGTH, E.REC_STEP, E.REC_TRUNCATED,
                                                                                                                E.REC_INFO, E.REC_EP_IM]
    keys = [f"k{j}" for j in range(E.INFO_DIM)]
    res = EV.EvalResult.from_ledger(counts, rec, 3, keys)
    assert res.episode_rewards == led.episode_rewards() and res.episode_lengths == led.episode_lengths()
    np.testing.assert_array_equal(res.env, led.column("env"))
    np.testing.assert_array_equal(res.step, led.column("step"))
    np.testing.assert_array_equal(res.truncated, led.column("truncated"))
    np.testing.assert_array_equal(res.policy, led.column("env") // 2)
    assert (res.mean_reward, res.std_reward) == led.mean_std() and res.mean_ep_length == float(np.mean(led.episode_lengths()))
    for j, k in enumerate(keys):
        np.testing.assert_array_equal(res.infos[k], led.column(j))
    parts = res.by_policy()
    assert len(parts) == 3
    for k, part in enumerate(parts):
        assert part.episode_rewards == led.episode_rewards(k) and len(part.episode_rewards) == 5 and (part.policy == k).all()
        assert (part.mean_reward, part.std_reward) == led.mean_std(k)
    s = res.summary(["k3", "ep_im_rew_mean"])
    assert s["n_episodes"] == 15 and s["k3"] == float(np.mean(led.column(3))) and s["mean_reward"] == res.mean_reward
    with pytest.raises(KeyError, match="nope"):
        res.summary(["nope"])


def test_descriptor_refusals():
    ok = dict(obs_cols=range(18), act_low=-np.ones(7), act_high=np.ones(7))
    d = EV.build_eval_desc(6, 3, 5, **ok)
    assert (d.n_envs, d.n_policies, d.n_eval_episodes, d.act_dim, d.n_obs_cols, d.goal_env, d.normalize) == (6, 3, 5, 7, 18, 0, 0)
    with pytest.raises(ValueError, match="not divisible by n_policies"):
        EV.build_eval_desc(7, 3, 5, **ok)
    with pytest.raises(ValueError, match="n_eval_episodes"):
        EV.build_eval_desc(6, 3, 0, **ok)
    limit = CONST["HRG_EVAL_MAX_EPISODES_PER_ENV"]
    EV.build_eval_desc(2, 1, 2 * limit, **ok)
    with pytest.raises(ValueError, match="HRG_EVAL_MAX_EPISODES_PER_ENV"):
        EV.build_eval_desc(2, 1, 2 * limit + 1, **ok)
    with pytest.raises(ValueError, match="mean and std come together"):
        EV.build_eval_desc(6, 1, 5, mean=np.zeros(18), **ok)
    with pytest.raises(ValueError, match="statistics of length"):
        EV.build_eval_desc(6, 1, 5, mean=np.zeros(18), std=np.ones(18), observe_time=True, **ok)
    with pytest.raises(NotImplementedError, match="feature row"):
        EV.build_eval_desc(6, 1, 5, goal_kind="reach", obs_cols=range(60), act_low=-np.ones(7), act_high=np.ones(7))
    with pytest.raises(NotImplementedError, match="plain selection"):
        EV.build_eval_desc(6, 1, 5, goal_kind="cube", observe_time=True, **ok)
    with pytest.raises(ValueError, match="finite, ordered"):
        EV.build_eval_desc(6, 1, 5, obs_cols=range(18), act_low=np.ones(7), act_high=-np.ones(7))
    g = EV.build_eval_desc(6, 1, 5, goal_kind="cube", obs_cols=range(7), act_low=-np.ones(4), act_high=np.ones(4))
    assert (g.goal_env, g.goal_kind, g.act_dim) == (1, CONST["HRG_GOAL_CUBE"], 4)


def test_evaluate_policy_refuses_what_the_device_loop_does_not_do():
    for kw, what in ((dict(deterministic=False), "deterministic=False"), (dict(render=True), "render"), (dict(callback=print), "callback")):
        with pytest.raises(NotImplementedError, match=what):
            EV.evaluate_policy(None, None, **kw)


def _sac_checkpoint(tmp_path, obs_dim=11, name="model_5.npz"):
    import torch
    from human_robot_gym_amd import sac
    desc = sac.build_sac_desc(obs_dim, 4, net_arch=[64, 64], batch_size=64, ent_coef="auto_0.2", seed=5)
    p = sac.SacParams(obs_dim, 4, 2, seed=5, ent_coef_init=0.2)
    g = torch.Generator().manual_seed(1)
    for t in (p.adam_m, p.adam_v, p.target):
        t.copy_(torch.rand(t.shape, generator=g))
    path = L.save_checkpoint(str(tmp_path / name), "hrg_sac", desc, p, (123, 2 ** 40 + 7), dict(learning_rate=5e-4))
    return path, desc, p


def test_checkpoint_round_trip_on_cpu_tensors(tmp_path):
    import torch
    from human_robot_gym_amd import sac
    path, desc, p = _sac_checkpoint(tmp_path)
    ck = L.load_checkpoint(path, "hrg_sac")
    assert [int(c) for c in ck["counters"]] == [123, 2 ** 40 + 7] and float(ck["hyper"]["learning_rate"]) == 5e-4
    for name, _ in desc._fields_:
        if not name.endswith("_"):
            assert ck["desc"][name] == getattr(desc, name), name
    assert float(ck["desc"]["ent_coef"]) == 0.2 and int(ck["desc"]["seed"]) == 5
    fresh = sac.SacParams(11, 4, 2, seed=9, ent_coef_init=1.0)
    assert not torch.equal(fresh.params, p.params)
    L.restore_tensors(fresh, ck)
    for name in L.TENSORS:
        assert torch.equal(getattr(fresh, name), getattr(p, name)), name
    # no pickle inside: the file loads with allow_pickle=False, and every entry is a plain array
    with np.load(path, allow_pickle=False) as f:
        assert all(f[k].dtype != object for k in f.files) and {"params", "adam_m", "adam_v", "target", "counters", "kind", "format"} <= set(f.files)


def test_a_checkpoint_of_another_shape_or_learner_is_refused_by_the_fields_name(tmp_path):
    from human_robot_gym_amd import sac
    path, _, _ = _sac_checkpoint(tmp_path)
    ck = L.load_checkpoint(path, "hrg_sac")
    with pytest.raises(ValueError, match="checkpoint: params is float32"):
        L.restore_tensors(sac.SacParams(12, 4, 2), ck)
    ck["target"] = ck["target"][:-1]
    with pytest.raises(ValueError, match="checkpoint: target"):
        L.restore_tensors(sac.SacParams(11, 4, 2), ck)
    with pytest.raises(ValueError, match="kind = 'hrg_sac'"):
        L.load_checkpoint(path, "hrg_ppo")
    other = str(tmp_path / "other.npz")
    np.savez(other, a=np.zeros(3))
    with pytest.raises(ValueError, match="format is missing"):
        L.load_checkpoint(other, "hrg_sac")


def test_checkpoint_names_are_the_references(tmp_path):
    assert TU.checkpoint_path("r1", 1_000_000) == os.path.join("models", "r1", "model_1_000_000.npz")
    assert TU.checkpoint_path("r1", 200000) == os.path.join("models", "r1", "model_200_000.npz")
    assert TU.checkpoint_path("r1", 0) == os.path.join("models", "r1", "model_0.npz")   # the reference refuses negative steps only
    assert TU.checkpoint_path("r1", 999) == os.path.join("models", "r1", "model_999.npz")
    assert TU.checkpoint_path("r1", "final", models_dir="m") == os.path.join("m", "r1", "model_final.npz")
    with pytest.raises(ValueError, match="non-negative integer or 'final'"):
        TU.checkpoint_path("r1", -1)
    with pytest.raises(ValueError, match="list_checkpoints"):
        TU.checkpoint_path("r1", "all")
    root = str(tmp_path)
    steps = [1_000_000, 200_000, 5, 30_000]
    for s in steps + ["final"]:
        path = TU.checkpoint_path("r1", s, models_dir=root)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        open(path, "wb").close()
    for stray in ("config.yaml", "model_final.zip", "model_x.npz", "notes_3.npz"):
        open(os.path.join(root, "r1", stray), "w").close()
    got = TU.list_checkpoints("r1", models_dir=root)
    assert [s for s, _ in got] == sorted(steps) + ["final"]
    assert [p for _, p in got] == [TU.checkpoint_path("r1", s, models_dir=root) for s in sorted(steps) + ["final"]]
    with pytest.raises(FileNotFoundError):
        TU.list_checkpoints("r2", models_dir=root)


def _namespace(node):
    return NS(**{k: _namespace(v) for k, v in node.items()}) if isinstance(node, dict) else node


@pytest.mark.parametrize("name", ["R-SAC", "PP-SAC", "CL-SAC"])
def test_eval_kwargs_from_the_icra_configs(name):
    import yaml
    cfg = yaml.safe_load(open(os.path.join(GOLDEN, name + ".yaml")))
    run = cfg["run"]
    for as_config in (dict(run=run), NS(run=_namespace(run))):
        kw = TU.eval_kwargs_from_config(as_config)
        assert kw == dict(n_eval_episodes=run["n_test_episodes"], log_info_keys=list(run["log_info_keys"]), eval_seed=run["eval_seed"])
    assert kw["n_eval_episodes"] == 20 and "n_goal_reached" in kw["log_info_keys"]
    assert TU.eval_kwargs_from_config(dict(run=dict(run, eval_seed=7)))["eval_seed"] == 7
    with pytest.raises(ValueError, match="n_test_episodes"):
        TU.eval_kwargs_from_config(dict(run=dict(run, n_test_episodes=0)))


def test_the_abi_declares_the_entries():
    want = ["hrg_eval_" + k for k in ("create", "destroy", "begin", "step", "policy_sac", "policy_ppo", "remaining", "export", "size")] + ["hrg_sac_restore", "hrg_ppo_restore"]
    assert all(k in PROTOTYPES for k in want), sorted(set(want) - set(PROTOTYPES))
    header = open(os.path.join(ROOT, "include", "hrgym.h")).read()
    assert re.search(r"typedef struct hrg_eval_desc \{", header) and "#define HRG_EVAL_MAX_EPISODES_PER_ENV" in header
    assert CONST["HRG_EVAL_RECORD_DIM"] == 5 + CONST["HRG_INFO_DIM"] and CONST["HRG_EVAL_REC_EP_IM"] == CONST["HRG_EVAL_RECORD_DIM"] - 1
    from human_robot_gym_amd._cstruct import EvalDesc
    assert [f for f, _ in EvalDesc._fields_][:3] == ["n_envs", "n_policies", "n_eval_episodes"]
    base = open(os.path.join(ROOT, "human-robot-gym_amd", "csrc", "hrgym_hip.hip")).read()
    assert base.index('#include "hrgym_ppo.h"') < base.index('#include "hrgym_eval.h"')
