"""Evaluate the checkpoints of a run on the device: the reference's `load_and_evaluate_model` (utils/training_utils_SB3.py:567-590) with `run.test_only`, for
the checkpoints the training tools write (`--model-dir models/<run_id>`).  One JSON line per checkpoint: mean / std of the deterministic policy's episode
returns over `--episodes` episodes (run.n_test_episodes), the mean episode length and the means of `--log-info-keys` at the episodes' last steps.

`--load-step all` (config_icra_2024/environment_evaluation/evaluation/*.yaml) evaluates every checkpoint of the run in ONE batch: the env count is rounded up
to a multiple of the number of checkpoints, and each group of envs steps its own parameter set (HipVecEnv.evaluate with a stacked parameter tensor).

The env is built from the command line -- the task, the horizon, the evaluation seed, `obs_keys`, a goal env for sac_her -- not from a run's config.yaml: a
checkpoint trained under `dataset_obs_norm`, an imitation reward or a dataset needs an env with those wrappers, which this tool cannot name.  For such a run
build the env with `training_utils.create_training_vec_env(config, evaluation_mode=True)` and call `env.evaluate` (INTEGRATION.md shows the lines).

python tools/evaluate.py --run-id 00042 --load-step all --algorithm sac --episodes 20"""
import argparse
import json
import sys

sys.path.insert(0, '.')
import torch   # noqa: E402
import human_robot_gym_amd as hrg   # noqa: E402
from human_robot_gym_amd.training_utils import checkpoint_path, list_checkpoints   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--run-id", required=True)
ap.add_argument("--load-step", default="final", help="an env step count, 'final', or 'all'")
ap.add_argument("--models-dir", default="models")
ap.add_argument("--algorithm", default="sac", choices=["sac", "sac_her", "ppo"])
ap.add_argument("--env-id", default="ReachHuman")
ap.add_argument("--obs-keys", nargs="+", default=None)
ap.add_argument("--n-envs", type=int, default=256)
ap.add_argument("--horizon", type=int, default=100)
ap.add_argument("--episodes", type=int, default=20, help="run.n_test_episodes, per checkpoint")
ap.add_argument("--eval-seed", type=int, default=1, help="run.eval_seed")
ap.add_argument("--log-info-keys", nargs="*", default=["n_goal_reached", "collision", "n_collisions", "timeout", "failsafe_interventions"])
ap.add_argument("--sync-every", type=int, default=16)
args = ap.parse_args()

if args.load_step == "all":
    checkpoints = list_checkpoints(args.run_id, models_dir=args.models_dir)
    if not checkpoints:
        raise SystemExit(f"no checkpoints under {args.models_dir}/{args.run_id}")
else:
    step = int(args.load_step) if args.load_step.replace("_", "").isdigit() else args.load_step
    checkpoints = [(step, checkpoint_path(args.run_id, step, models_dir=args.models_dir))]
from human_robot_gym_amd.ppo import PpoLearner   # noqa: E402
from human_robot_gym_amd.sac import SacLearner   # noqa: E402
cls = PpoLearner if args.algorithm == "ppo" else SacLearner
learners = [cls.load(path, device=0) for _, path in checkpoints]
first = learners[0]
for (step, path), learner in zip(checkpoints, learners):
    if learner.p.n_params != first.p.n_params or (learner.obs_dim, learner.act_dim, learner.depth) != (first.obs_dim, first.act_dim, first.depth):
        raise SystemExit(f"{path}: a learner of other shapes than {checkpoints[0][1]}: one batch steps parameter sets of one shape")
P = len(learners)
n_envs = -(-args.n_envs // P) * P   # a multiple of the number of checkpoints
# create_training_vec_env(config, evaluation_mode=True): the env of the run with the evaluation seed
kw = dict(env_id=args.env_id, env_kwargs=dict(horizon=args.horizon, seed=args.eval_seed))
if args.algorithm == "sac_her":
    kw.update(goal_env=True, obs_keys=args.obs_keys or ["object-state", "robot0_joint_pos"])
elif args.obs_keys is not None:
    kw.update(obs_keys=args.obs_keys)
env = hrg.HipVecEnv(n_envs, **kw)
result = env.evaluate(torch.stack([learner.p.params for learner in learners]).contiguous(), args.episodes, sync_every=args.sync_every, learner=first)
for (step, path), part in zip(checkpoints, result.by_policy()):
    line = dict(run_id=args.run_id, load_step=step, checkpoint=path, n_envs=n_envs // P)
    line.update(part.summary(args.log_info_keys))
    print(json.dumps(line), flush=True)
env.close()
