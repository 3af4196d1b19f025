"""`create_training_vec_env(config, evaluation_mode)` — the reference's env construction for a training run
(utils/training_utils_SB3.py:45-77), returning the batched HIP VecEnv instead of a SubprocVecEnv.

The reference builds `wrapper_class = get_environment_wrap_fn(config)` (utils/training_utils.py:350-410: per-env gym wrappers chosen by
`config.wrappers.*`) and hands it to `make_vec_env`.  Per-env Python wrappers cannot wrap a batch that lives on the GPU, so the
wrappers the stepper implements in its kernels are read from the same config nodes instead:

  config.wrappers.collision_prevention  -> CollisionPreventionWrapper (wrappers/collision_prevention_wrapper.py) in the step kernel's prologue
  config.wrappers.ik_position_delta     -> IKPositionDeltaWrapper (wrappers/ik_position_delta_wrapper.py) in the step kernel's prologue
  config.wrappers.dataset_obs_norm      -> DatasetObsNormWrapper (wrappers/dataset_wrapper.py:160-300) on the host, when the statistics are
                                           given (mean / std in the config, or datasets/<name>/observations.csv)
  config.wrappers.action_based_expert_imitation_reward with alpha == 0 and rsi_prob == 0 (the *-SAC baselines of config_icra_2024): the
                                           wrapper then returns the environment reward unchanged and never resets to a dataset state; it is skipped
  config.wrappers.action_based_expert_imitation_reward with rsi_prob: null and a config.expert node (the *-AIR configs with that one key set to
                                           null) -> the scripted expert + Cart/JointActionBasedExpertImitationRewardWrapper in two kernels around
                                           the step kernel (HipVecEnv expert= / imitation_reward=; csrc/hrgym_expert.h)
  config.wrappers.state_based_expert_imitation_reward, and action_based_expert_imitation_reward with a non-null rsi_prob, when
                                           datasets/<dataset_name>/hrg_dataset.npz exists (tools/create_expert_dataset.py records one) -> the dataset on
                                           the device: every episode starts from one of its states, and the state based reward compares the state reached
                                           with the demonstration's (HipVecEnv dataset= / rsi_prob= / state_imitation_reward=; csrc/hrgym_dataset.h)
  anything else that is configured (an imitation wrapper whose dataset file does not exist, visualisation) raises.

`config` may be the reference's OmegaConf `TrainingConfig`, or any object / dict with the same attribute tree (the tests use a plain namespace).
"""
import csv
import os
from argparse import Namespace
from types import SimpleNamespace
from typing import Any, Dict, Optional

import numpy as np

from .env_util import make_vec_env


def _get(node, name, default=None):
    if node is None:
        return default
    if isinstance(node, dict):
        return node.get(name, default)
    try:
        v = getattr(node, name)
    except Exception:  # noqa: BLE001  (OmegaConf raises its own errors for missing keys)
        try:
            return node[name]
        except Exception:  # noqa: BLE001
            return default
    return v


def _plain(node):
    """OmegaConf node / namespace / dict -> plain dicts and lists (OmegaConf.to_container(resolve=True) when available)."""
    if node is None or isinstance(node, (str, int, float, bool)):
        return node
    try:  # pragma: no cover - omegaconf is not installed in the build container
        from omegaconf import OmegaConf
        if OmegaConf.is_config(node):
            return OmegaConf.to_container(node, resolve=True, throw_on_missing=True)
    except ImportError:
        pass
    if isinstance(node, dict):
        return {k: _plain(v) for k, v in node.items()}
    if isinstance(node, (list, tuple)):
        return [_plain(v) for v in node]
    if isinstance(node, (SimpleNamespace, Namespace)):
        return {k: _plain(v) for k, v in vars(node).items() if not k.startswith("_")}
    return node   # any other object (a ClipSet, a backend factory, ...) is a value, not a config node


def compose_environment_kwargs(config, evaluation_mode: bool = False) -> Dict[str, Any]:
    """utils/training_utils.py:71-88 (`_compose_environment_kwargs`): config.environment without env_id, + robots, + the evaluation seed.
    `controller_configs` is not composed: the stepper's controller is failsafe.json + schunk.json, compiled into the model description."""
    kwargs = dict(_plain(_get(config, "environment")) or {})
    kwargs.pop("env_id", None)
    kwargs["robots"] = _get(_get(config, "robot"), "name", "Schunk")
    if evaluation_mode and _get(_get(config, "run"), "eval_seed") is not None:
        kwargs["seed"] = _get(_get(config, "run"), "eval_seed")
    return kwargs


def _obs_norm_from_config(node) -> Optional[Dict[str, Any]]:
    kw = dict(_plain(node))
    mean, std = kw.get("mean"), kw.get("std")
    if mean is None or std is None:
        path = os.path.join("datasets", str(kw.get("dataset_name")), "observations.csv")   # dataset_wrapper.py:213-216
        if not os.path.exists(path):
            raise NotImplementedError(f"wrappers.dataset_obs_norm: no mean/std in the config and no {path}; computing the statistics from the pickled "
                                      "dataset (dataset_wrapper.py:217-221) is not supported")
        with open(path, newline="") as f:
            rows = list(csv.DictReader(f))
        mean = [float(r["mean"]) for r in rows] if mean is None else mean
        std = [float(r["std"]) for r in rows] if std is None else std
    return dict(mean=np.asarray(mean, np.float64), std=np.asarray(std, np.float64), squash_factor=kw.get("squash_factor"),
                allow_different_observation_shapes=bool(kw.get("allow_different_observation_shapes", False)))


def _dataset_file(name) -> str:
    return os.path.join("datasets", str(name), "hrg_dataset.npz")   # dataset.dataset_path: relative to the working directory, like observations.csv above


def _dataset_file_exists(name) -> bool:
    return name is not None and os.path.exists(_dataset_file(name))


def wrapper_kwargs_from_config(config) -> Dict[str, Any]:
    """`get_environment_wrap_fn(config)` (utils/training_utils.py:350-410), translated into HipVecEnv keyword arguments."""
    w = _get(config, "wrappers")
    out: Dict[str, Any] = {}
    cp = _get(w, "collision_prevention")
    if cp is not None:
        out["collision_prevention"] = dict(_plain(cp))
    ik = _get(w, "ik_position_delta")
    if ik is not None:   # env_has_cartesian_action_space (training_utils.py:204-206); kwargs as _compose_ik_position_delta_wrapper_kwargs (177-201)
        ikw = dict(_plain(ik))
        ikw.pop("urdf_file", None)   # the kernel's chain is the stepper's own model of robot_pybullet.urdf
        out["ik_position_delta"] = ikw
    sb = _get(w, "state_based_expert_imitation_reward")
    if sb is not None:   # state_based_expert_imitation_reward_wrap_fn (training_utils.py): the wrapper of the task, on a dataset recorded for the batched stepper
        sbk = dict(_plain(sb))
        name, rsi_prob = sbk.pop("dataset_name", None), sbk.pop("rsi_prob", 0.0)
        if not _dataset_file_exists(name):
            raise NotImplementedError(f"wrappers.state_based_expert_imitation_reward: the wrapper compares with the states of a recorded dataset and no "
                                      f"{_dataset_file(name)} exists for the batched stepper (the reference's per-episode folders are not read; record one "
                                      "with tools/create_expert_dataset.py)")
        out["dataset"], out["rsi_prob"], out["state_imitation_reward"] = str(name), float(rsi_prob or 0.0), sbk
    ab = _get(w, "action_based_expert_imitation_reward")
    if ab is not None:
        abk = dict(_plain(ab))
        rsi_prob = abk.pop("rsi_prob", None)
        name = abk.pop("dataset_name", None)   # _compose_action_based_expert_imitation_reward_wrapper_kwargs (training_utils.py:252-271)
        expert = _get(config, "expert")
        rsi = rsi_prob is not None and _dataset_file_exists(name)
        if rsi:   # action_based_expert_imitation_reward_wrap_fn (training_utils.py:297-307) wraps DatasetRSIWrapper whenever rsi_prob is not None
            if "dataset" in out:
                raise NotImplementedError("wrappers: state_based_ and action_based_expert_imitation_reward together (the reference wraps one of them)")
            out["dataset"], out["rsi_prob"] = str(name), float(rsi_prob)
        if rsi_prob is not None and not rsi:
            if float(abk.get("alpha") or 0.0) != 0.0 or float(rsi_prob) != 0.0:
                raise NotImplementedError(f"wrappers.action_based_expert_imitation_reward with rsi_prob = {rsi_prob}: the reference then wraps DatasetRSIWrapper, "
                                          f"which resets episodes to the states of a recorded dataset; no {_dataset_file(name)} exists "
                                          "for the batched stepper (tools/create_expert_dataset.py records one).  Set rsi_prob to null for the imitation reward alone (alpha = 0, rsi_prob = 0 leaves the "
                                          "environment reward unchanged and is skipped)")
        elif expert is None:
            if float(abk.get("alpha") or 0.0) != 0.0:   # alpha = 0 without an expert: the environment reward unchanged; skipped as before
                raise NotImplementedError("wrappers.action_based_expert_imitation_reward without a config.expert node (the reference asserts: No expert specified in config!)")
        else:
            from .expert import EXPERT_ENVS, expert_kwargs
            ek = dict(_plain(expert))   # _compose_expert_kwargs / create_expert (training_utils.py:138-174): id selects the class, obs_keys is dropped
            ek.pop("obs_keys", None)
            # (every other expert on a task it does not fit is refused when the env is built, HipVecEnv._check_expert; this one also before its arguments are read)
            if ek.get("id") == "ReachHumanCart" and _get(_get(config, "environment"), "env_id") not in EXPERT_ENVS["ReachHumanCart"]:
                raise NotImplementedError("expert ReachHumanCart reads the goal_difference of the ReachHumanCart environment only (config.environment.env_id)")
            expert_kwargs(ek)           # unknown ids and arguments raise now, not at the first step
            out["expert"] = ek
            out["imitation_reward"] = abk
    dn = _get(w, "dataset_obs_norm")
    if dn is not None:
        out["obs_norm"] = _obs_norm_from_config(dn)
    if _get(w, "visualization") is not None:
        raise NotImplementedError("wrappers.visualization: the batched stepper has no renderer")
    return out


def her_kwargs_from_config(config) -> Optional[Dict[str, Any]]:
    """`config.algorithm.replay_buffer_kwargs` of a goal-env run (training/config/algorithm/sac_her.yaml: n_sampled_goal, goal_selection_strategy,
    online_sampling) -> the keyword arguments of HipVecEnv.attach_her, or None when the run has no such node.  `buffer_size` is per env there: the
    algorithm's buffer_size (transitions in all) divided over run.n_envs, but never less than two episodes."""
    run, alg = _get(config, "run"), _get(config, "algorithm")
    node = _get(alg, "replay_buffer_kwargs")
    if node is None or _get(run, "env_type", "env") != "goal_env":
        return None
    kw = dict(_plain(node))
    unknown = sorted(set(kw) - {"n_sampled_goal", "goal_selection_strategy", "online_sampling", "max_episode_length", "handle_timeout_termination"})
    if unknown:
        raise NotImplementedError(f"algorithm.replay_buffer_kwargs {unknown}: the device buffer takes n_sampled_goal, goal_selection_strategy, online_sampling")
    if kw.pop("handle_timeout_termination", True) is not True:
        raise NotImplementedError("algorithm.replay_buffer_kwargs.handle_timeout_termination = false: the device buffer never stores a timeout as a termination")
    kw.pop("max_episode_length", None)   # the horizon of the env
    horizon = int(_get(_get(config, "environment"), "horizon", 0) or 0)
    n_envs = int(_get(run, "n_envs", 1))
    total = int(_get(alg, "buffer_size", 1_000_000))
    kw["buffer_size"] = max(total // n_envs, 2 * horizon + 2)
    return kw


def rollout_kwargs_from_config(config) -> Optional[Dict[str, Any]]:
    """`config.algorithm` of an on-policy run (training/config/algorithm/ppo.yaml: name PPO, n_steps, gamma, gae_lambda) on flat observations
    (run.env_type "env") -> the keyword arguments of HipVecEnv.attach_rollout; None for any other config.  Missing keys take SB3's PPO defaults."""
    run, alg = _get(config, "run"), _get(config, "algorithm")
    if str(_get(alg, "name", "")).upper() != "PPO" or _get(run, "env_type", "env") != "env":
        return None
    return dict(n_steps=int(_get(alg, "n_steps", 2048)), gamma=float(_get(alg, "gamma", 0.99)), gae_lambda=float(_get(alg, "gae_lambda", 0.95)))


def replay_kwargs_from_config(config) -> Optional[Dict[str, Any]]:
    """`config.algorithm` of an off-policy run on flat observations (training/config_icra_2024/.../*-SAC.yaml: name SAC, buffer_size; run.env_type "env")
    -> the keyword arguments of HipVecEnv.attach_replay; None for any other config (a goal-env run's buffer is her_kwargs_from_config's).  `buffer_size` is
    the algorithm's, transitions in all (SB3's default 1 000 000).  optimize_memory_usage and replay_buffer_kwargs.handle_timeout_termination are handed on
    where the config sets them, so that attach_replay refuses what the device buffer does not do."""
    run, alg = _get(config, "run"), _get(config, "algorithm")
    if str(_get(alg, "name", "")).upper() != "SAC" or _get(run, "env_type", "env") != "env":
        return None
    kw: Dict[str, Any] = dict(buffer_size=int(_get(alg, "buffer_size", 1_000_000)))
    if _get(alg, "optimize_memory_usage") is not None:
        kw["optimize_memory_usage"] = bool(_get(alg, "optimize_memory_usage"))
    node = _plain(_get(alg, "replay_buffer_kwargs")) or {}
    if "handle_timeout_termination" in node:
        kw["handle_timeout_termination"] = bool(node["handle_timeout_termination"])
    return kw


def sac_kwargs_from_config(config) -> Dict[str, Any]:
    """`config.algorithm` of a SAC run (training/config_icra_2024/.../*-SAC.yaml) -> the keyword arguments of HipVecEnv.attach_sac / sac.SacLearner:
    net_arch, learning_rate, gamma, tau, ent_coef, target_entropy, batch_size, target_update_interval, seed (missing keys take SB3's SAC defaults).
    What the kernels do not cover is refused by the name of its key: use_sde, action_noise, policy, policy_kwargs.net_arch.  `policy`: MlpPolicy, or
    MultiInputPolicy exactly when run.env_type is goal_env (training/config/algorithm/sac_her.yaml); the result carries it for a goal env.  train_freq --
    sac_her.yaml's [1, episode] included, which SB3 1.5.0 itself forbids with more than one env --, gradient_steps, learning_starts, buffer_size and
    replay_buffer_kwargs belong to the loop and the buffer (tools/train_sac.py, tools/train_sac_her.py, replay_kwargs_from_config, create_training_vec_env),
    not to the learner."""
    alg = _get(config, "algorithm")
    if str(_get(alg, "name", "SAC")).upper() != "SAC":
        raise NotImplementedError(f"algorithm.name = {_get(alg, 'name')}: the device learner is SAC")
    from .sac import check_policy
    goal_env = _get(_get(config, "run"), "env_type", "env") == "goal_env"
    try:
        policy = check_policy(_get(alg, "policy"), goal_env)
    except NotImplementedError as e:
        raise NotImplementedError(f"algorithm.policy with run.env_type = {'goal_env' if goal_env else 'env'}: {e}") from None
    if _get(alg, "use_sde", False):
        raise NotImplementedError("algorithm.use_sde = true: state dependent exploration is not covered by the device learner")
    if _get(alg, "action_noise") is not None:
        raise NotImplementedError("algorithm.action_noise: the device learner adds no action noise")
    from .sac import depth_of
    pk = _plain(_get(alg, "policy_kwargs")) or {}
    net_arch = pk.get("net_arch", [256, 256])   # SB3's default for SAC
    try:
        depth_of(net_arch)
    except NotImplementedError as e:
        raise NotImplementedError(f"algorithm.policy_kwargs.net_arch: {e}") from None
    unknown = sorted(set(pk) - {"net_arch"})
    if unknown:
        raise NotImplementedError(f"algorithm.policy_kwargs {unknown}: the device learner takes net_arch")
    kw: Dict[str, Any] = dict(net_arch=[int(w) for w in net_arch], learning_rate=float(_get(alg, "learning_rate", 3e-4)), gamma=float(_get(alg, "gamma", 0.99)),
                              tau=float(_get(alg, "tau", 0.005)), ent_coef=_get(alg, "ent_coef", "auto"), target_entropy=_get(alg, "target_entropy", "auto"),
                              batch_size=int(_get(alg, "batch_size", 256)), target_update_interval=int(_get(alg, "target_update_interval", 1)))
    if _get(alg, "seed") is not None:
        kw["seed"] = int(_get(alg, "seed"))
    if goal_env:
        kw["policy"] = policy
    return kw


def ppo_kwargs_from_config(config) -> Dict[str, Any]:
    """`config.algorithm` of a PPO run (training/config/algorithm/ppo.yaml) -> the keyword arguments of HipVecEnv.attach_ppo / ppo.PpoLearner: net_arch,
    learning_rate, batch_size, n_epochs, clip_range, clip_range_vf, normalize_advantage, ent_coef, vf_coef, max_grad_norm, log_std_init, ortho_init, seed
    (missing keys take SB3's PPO defaults).  What the kernels do not cover is refused by the name of its key: use_sde, target_kl, policy,
    policy_kwargs.net_arch, any other policy_kwargs key.  policy_kwargs.full_std, use_expln and squash_output are dropped: in SB3 1.5.0 they reach gSDE and
    predict() only.  n_steps, gamma and gae_lambda belong to the buffer (rollout_kwargs_from_config), sde_sample_freq to gSDE."""
    alg = _get(config, "algorithm")
    if str(_get(alg, "name", "PPO")).upper() != "PPO":
        raise NotImplementedError(f"algorithm.name = {_get(alg, 'name')}: the device learner is PPO")
    if _get(alg, "policy", "MlpPolicy") != "MlpPolicy":
        raise NotImplementedError(f"algorithm.policy = {_get(alg, 'policy')}: the device learner covers MlpPolicy")
    if _get(alg, "use_sde", False):
        raise NotImplementedError("algorithm.use_sde = true: state dependent exploration is not covered by the device learner")
    if _get(alg, "target_kl") is not None:
        raise NotImplementedError(f"algorithm.target_kl = {_get(alg, 'target_kl')}: the early stop needs a host readback per minibatch; the device learner runs every epoch")
    from .ppo import IGNORED_POLICY_KWARGS, parse_net_arch
    pk = _plain(_get(alg, "policy_kwargs")) or {}
    net_arch = pk.get("net_arch", [dict(pi=[64, 64], vf=[64, 64])])   # SB3's default for an ActorCriticPolicy
    try:
        parse_net_arch(net_arch)
    except NotImplementedError as e:
        raise NotImplementedError(f"algorithm.policy_kwargs.net_arch: {e}") from None
    unknown = sorted(set(pk) - {"net_arch", "log_std_init", "ortho_init"} - set(IGNORED_POLICY_KWARGS))
    if unknown:
        raise NotImplementedError(f"algorithm.policy_kwargs {unknown}: the device learner takes net_arch, log_std_init and ortho_init")
    clip_range_vf = _get(alg, "clip_range_vf")
    kw: Dict[str, Any] = dict(net_arch=net_arch, learning_rate=float(_get(alg, "learning_rate", 3e-4)), batch_size=int(_get(alg, "batch_size", 64)),
                              n_epochs=int(_get(alg, "n_epochs", 10)), clip_range=float(_get(alg, "clip_range", 0.2)),
                              clip_range_vf=None if clip_range_vf is None else float(clip_range_vf), normalize_advantage=bool(_get(alg, "normalize_advantage", True)),
                              ent_coef=float(_get(alg, "ent_coef", 0.0)), vf_coef=float(_get(alg, "vf_coef", 0.5)), max_grad_norm=float(_get(alg, "max_grad_norm", 0.5)),
                              log_std_init=float(pk.get("log_std_init", 0.0)), ortho_init=bool(pk.get("ortho_init", True)))
    if _get(alg, "seed") is not None:
        kw["seed"] = int(_get(alg, "seed"))
    return kw


CHECKPOINT_EXT = ".npz"   # a device learner's checkpoint (Learner.save), where the reference writes SB3's .zip


def checkpoint_path(run_id, load_step, models_dir="models") -> str:
    """`models/<run_id>/model_<step>` of the reference (utils/training_utils_SB3.py:240-243; callbacks/custom_wandb_callback.py writes the same names): an
    integer step with `_` between the thousands (model_1_000_000), anything else as it is (model_final); the extension is a device checkpoint's."""
    if isinstance(load_step, bool) or (isinstance(load_step, int) and load_step < 0):
        raise ValueError("load_step must be a non-negative integer or 'final'")   # (the reference's check, load_step < 0, under its own wording "positive")
    if not isinstance(load_step, int) and str(load_step) == "all":
        raise ValueError("load_step 'all' names every checkpoint of the run: list_checkpoints(run_id)")
    name = f"model_{load_step:_}" if isinstance(load_step, int) else f"model_{load_step}"
    return os.path.join(models_dir, str(run_id), name + CHECKPOINT_EXT)


def list_checkpoints(run_id, models_dir="models"):
    """`load_step: all` (config_icra_2024/environment_evaluation/evaluation/*.yaml): [(step, path)] of every checkpoint of the run, by ascending step;
    model_final, where it exists, comes last under the step "final"."""
    folder = os.path.join(models_dir, str(run_id))
    if not os.path.isdir(folder):
        raise FileNotFoundError(f"{folder}: no such run")
    steps, final = [], []
    for f in os.listdir(folder):
        stem, ext = os.path.splitext(f)
        if ext != CHECKPOINT_EXT or not stem.startswith("model_"):
            continue
        tag = stem[len("model_"):]
        if tag == "final":
            final.append(("final", os.path.join(folder, f)))
        elif tag.replace("_", "").isdigit():
            steps.append((int(tag.replace("_", "")), os.path.join(folder, f)))
    return sorted(steps) + final


def eval_kwargs_from_config(config) -> Dict[str, Any]:
    """`config.run` of an evaluation (utils/training_utils_SB3.py:492-544) -> dict(n_eval_episodes = run.n_test_episodes, log_info_keys = run.log_info_keys,
    eval_seed = run.eval_seed): the first is HipVecEnv.evaluate's argument, the second EvalResult.summary's, the third is what
    create_training_vec_env(config, evaluation_mode=True) seeds the env with (None: the training seed)."""
    run = _get(config, "run")
    n = _get(run, "n_test_episodes")
    if n is None or int(n) < 1:
        raise ValueError(f"run.n_test_episodes = {n}: a positive number of evaluation episodes")
    seed = _get(run, "eval_seed")
    return dict(n_eval_episodes=int(n), log_info_keys=[str(k) for k in (_plain(_get(run, "log_info_keys")) or [])], eval_seed=None if seed is None else int(seed))


class RunFolder:
    """What a training loop of the tools does to `models/<run_id>` (utils/training_utils_SB3.py:399-461, callbacks/custom_wandb_callback.py): a checkpoint
    whenever the env steps pass another multiple of `save_freq`, `model_final` at the end, and -- with `eval_env` and `eval_episodes` -- an evaluation of
    the learner after every block, whose figures `after` returns for the block's log line.  With neither `model_dir` nor `eval_episodes` every call is a no-op."""

    def __init__(self, model_dir=None, save_freq=None, eval_env=None, eval_episodes=0):
        self.model_dir, self.save_freq, self.eval_env, self.eval_episodes = model_dir, int(save_freq or 0), eval_env, int(eval_episodes or 0)
        self._saved_until = 0

    def path(self, step):
        folder = os.path.abspath(self.model_dir)
        return checkpoint_path(os.path.basename(folder), step, models_dir=os.path.dirname(folder))

    def after(self, learner, env_steps) -> Dict[str, Any]:
        out: Dict[str, Any] = {}
        if self.model_dir is not None and self.save_freq > 0 and env_steps // self.save_freq > self._saved_until:
            self._saved_until = env_steps // self.save_freq
            out["checkpoint"] = learner.save(self.path(int(env_steps)))
        if self.eval_env is not None and self.eval_episodes > 0:
            res = self.eval_env.evaluate(learner, self.eval_episodes)
            out.update(eval_mean_reward=res.mean_reward, eval_std_reward=res.std_reward, eval_mean_ep_length=res.mean_ep_length)
        return out

    def finish(self, learner):
        return None if self.model_dir is None else learner.save(self.path("final"))


def sweep_members(sweeps, seeds, n_envs, fields, max_members):
    """The members of a training tool's --sweep NAME=v1,v2,... (repeatable) and --seeds: the values of every sweep crossed with each other and with the seeds,
    value-major and seed-minor (the first sweep's value changes slowest, the seed fastest) -> (seeds [P], {name: values [P]}).  A value is a float where it
    reads as one, None for "none", otherwise the string itself ("auto_0.2").  ValueError, before any env is built: an option that is no NAME=v1,v2,..., a name
    that is no per-member field (`fields`) or given twice, more than `max_members` members, `n_envs` that the members do not divide."""
    from itertools import product

    def value(text):
        if text.strip().lower() == "none":
            return None
        try:
            return float(text)
        except ValueError:
            return text.strip()

    names, lists = [], []
    for opt in sweeps or ():
        name, sep, rest = str(opt).partition("=")
        name = name.strip().replace("-", "_")
        if not sep or not name or not rest.strip() or any(not v.strip() for v in rest.split(",")):
            raise ValueError(f"--sweep {opt}: expected NAME=v1,v2,...")
        if name not in fields:
            raise ValueError(f"--sweep {opt}: {name} is no per-member field (those are {', '.join(fields)}); what shapes a launch or the lockstep is shared by the members")
        if name in names:
            raise ValueError(f"--sweep {opt}: {name} is swept twice")
        names.append(name)
        lists.append([value(v) for v in rest.split(",")])
    seeds = [int(s) for s in seeds]
    members = list(product(*lists, seeds))
    P = len(members)
    if not 1 <= P <= int(max_members):
        raise ValueError(f"{' x '.join(str(len(v)) for v in lists + [seeds])} = {P} members: a population has 1 .. {int(max_members)}")
    if int(n_envs) % P:
        raise ValueError(f"--n-envs {n_envs} is not divisible by the {P} members: every member steps a group of the same size")
    return [m[-1] for m in members], {name: [m[i] for m in members] for i, name in enumerate(names)}


def checked_sweep(population, sweeps, seeds, n_envs, max_members):
    """sweep_members for the fields of the population class `population`, with every swept value checked as its constructor checks it
    (Population.member_values): a value no learner takes (gamma=nan, learning_rate=-1) is refused here, before any env is built, too."""
    seeds, swept = sweep_members(sweeps, seeds, n_envs, population._fields, max_members)
    population.member_values(len(seeds), **swept)
    return seeds, swept


def member_lines(seeds, swept, *parts):
    """The `members` list of a population's JSON line: per member dict(seed, **its entry of every list of dicts in `parts` -- episode stats, diagnostics) and, where
    something is swept, `hyper`: the member's value of every swept field.  The values stand under a key of their own because the diagnostics report
    `learning_rate`, `clip_range` and the live `ent_coef` under the fields' own names."""
    lines = []
    for p, seed in enumerate(seeds):
        line = dict(seed=seed)
        if swept:
            line["hyper"] = {name: values[p] for name, values in swept.items()}
        for part in parts:
            line.update(part[p])
        lines.append(line)
    return lines


def run_folder_from_args(args, **env_kw) -> RunFolder:
    """The RunFolder of a training tool's --model-dir / --save-freq / --eval-episodes / --eval-n-envs / --eval-seed, with a second env of the tool's task for
    the evaluations (its own seed: the reference's eval_seed; `env_kw`: further HipVecEnv keywords).  Without the flags nothing is built."""
    eval_env = None
    if args.eval_episodes > 0:
        from .vec_env import HipVecEnv
        seed = args.seed + 1 if args.eval_seed is None else args.eval_seed
        eval_env = HipVecEnv(args.eval_n_envs, env_id=args.env_id, env_kwargs=dict(horizon=args.horizon, seed=seed), **env_kw)
    return RunFolder(args.model_dir, args.save_freq, eval_env, args.eval_episodes)


def create_training_vec_env(config, evaluation_mode: bool = False, wrapper_class=None):
    """Drop-in for `human_robot_gym.utils.training_utils_SB3.create_training_vec_env` (45-77).  `wrapper_class`, when given (the reference always
    builds one from the same config), is accepted and not called: what it would have wrapped is read from `config.wrappers` here."""
    run = _get(config, "run")
    env_kwargs = compose_environment_kwargs(config, evaluation_mode)
    vec_kw = dict(_plain(_get(run, "vec_env_kwargs")) or {})
    vec_kw.update(wrapper_kwargs_from_config(config))
    vec_kw["_wrappers_from_config"] = True   # tells make_vec_env that `wrapper_class` (if any) has been translated above
    her = her_kwargs_from_config(config)
    env = make_vec_env(
        env_id=_get(_get(config, "environment"), "env_id"),
        type=_get(run, "env_type", "env"),
        obs_keys=_plain(_get(run, "obs_keys")),
        expert_obs_keys=_plain(_get(run, "expert_obs_keys")),
        n_envs=int(_get(run, "n_envs", 1)),
        seed=_get(run, "seed"),
        start_index=int(_get(run, "start_index", 0) or 0),
        monitor_dir=_get(run, "monitor_dir"),
        wrapper_class=wrapper_class,
        env_kwargs=env_kwargs,
        vec_env_cls=None,
        vec_env_kwargs=vec_kw,
        monitor_kwargs=_plain(_get(run, "monitor_kwargs")),
        wrapper_kwargs=None,
    )
    if her is not None:   # SAC + HER: the replay buffer lives beside the stepper (env.her)
        if her["buffer_size"] <= env.horizon:
            her["buffer_size"] = 2 * env.horizon + 2
        env.attach_her(**her)
    rollout = rollout_kwargs_from_config(config)
    # PPO: the rollout buffer lives beside the stepper (env.rollout, env.collect_rollout).  Only where the device path covers the env: another backend, or a
    # wrapper that works on the host path (obs_norm, a dataset, an imitation reward), trains through step() as before
    if rollout is not None and env.device_refusal("rollout") is None:
        env.attach_rollout(**rollout)
    replay = replay_kwargs_from_config(config)
    # SAC on flat observations: the replay buffer lives beside the stepper (env.replay, env.collect_steps), with the wrappers of the config on; another
    # backend and the mixed batch train through step() as before
    if replay is not None and env.device_refusal("replay") is None:
        env.attach_replay(**replay)
    return env
