"""The whole SAC alternation on one GPU, nothing leaving the device between the blocks: `env.collect_steps(learner.act, train_freq)`, then
`learner.train(env.replay, gradient_steps)`; uniform random actions until `learning_starts` transitions are stored (SB3's warm-up).  One JSON line per block:
`env.replay.episode_stats()` and `learner.diagnostics()`.  A demonstration of the plumbing; it carries no claim about learning curves.

--gradient-steps is explicit.  The ICRA configs say `train_freq: [100, step]`, `gradient_steps: -1`: in SB3 1.5.0 -1 means "as many gradient steps as
transitions were collected in the rollout", train_freq * n_envs.  With 8 envs that is 800 per block; with 4096 it would be 409 600: whether a run at thousands of
envs keeps that ratio is the user's decision.

python tools/train_sac.py --n-envs 1024 --gradient-steps 800 --blocks 20"""
import argparse
import json
import sys
import time

sys.path.insert(0, '.')
import torch   # noqa: E402
import human_robot_gym_amd as hrg   # noqa: E402
from human_robot_gym_amd.training_utils import run_folder_from_args   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--env-id", default="ReachHuman")
ap.add_argument("--n-envs", type=int, default=1024)
ap.add_argument("--horizon", type=int, default=100)
ap.add_argument("--train-freq", type=int, default=100, help="env steps (of every env) per block")
ap.add_argument("--gradient-steps", type=int, required=True, help="gradient steps per block")
ap.add_argument("--blocks", type=int, default=10)
ap.add_argument("--learning-starts", type=int, default=1000, help="transitions stored before the first gradient step; uniform random actions until then")
ap.add_argument("--buffer-size", type=int, default=1_000_000)
ap.add_argument("--batch-size", type=int, default=128)
ap.add_argument("--learning-rate", type=float, default=5e-4)
ap.add_argument("--ent-coef", default="auto_0.2")
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--model-dir", default=None, help="models/<run_id>: checkpoints model_<step>.npz every --save-freq env steps and model_final.npz at the end")
ap.add_argument("--save-freq", type=int, default=0, help="env steps between checkpoints (with --model-dir)")
ap.add_argument("--eval-episodes", type=int, default=0, help="evaluate the deterministic policy on a second env after every block (n_test_episodes)")
ap.add_argument("--eval-n-envs", type=int, default=64)
ap.add_argument("--eval-seed", type=int, default=None, help="seed of the evaluation env (default: --seed + 1)")
args = ap.parse_args()

env = hrg.HipVecEnv(args.n_envs, env_id=args.env_id, env_kwargs=dict(horizon=args.horizon, seed=args.seed))
env.attach_replay(args.buffer_size)
learner = env.attach_sac(batch_size=args.batch_size, learning_rate=args.learning_rate, ent_coef=args.ent_coef, seed=args.seed)
gen = torch.Generator(device=learner.device).manual_seed(args.seed)


def uniform(obs):
    return torch.rand(obs.shape[0], learner.act_dim, generator=gen, device=obs.device) * 2.0 - 1.0


run = run_folder_from_args(args)
t0 = time.time()
for block in range(args.blocks):
    stored = env.replay.size() * args.n_envs
    warm = stored < args.learning_starts
    env.collect_steps(uniform if warm else learner.act, args.train_freq)
    if env.replay.size() * args.n_envs >= args.learning_starts:
        learner.train(env.replay, args.gradient_steps)
    line = dict(block=block, env_steps=(block + 1) * args.train_freq * args.n_envs, policy="uniform" if warm else "actor", seconds=round(time.time() - t0, 3))
    line.update(env.replay.episode_stats())
    if learner.n_updates:
        line.update(learner.diagnostics())
    line.update(run.after(learner, line["env_steps"]))
    print(json.dumps(line), flush=True)
run.finish(learner)
env.close()
