"""The whole PPO alternation on one GPU, nothing leaving the device between the rollouts: `env.collect_rollout(learner.policy, learner.value)`, then
`learner.train(env.rollout)` -- n_epochs passes over the buffer in minibatches of batch_size.  One JSON line per rollout: `env.rollout.episode_stats()` and
`learner.diagnostics()`.  The defaults are training/config/algorithm/ppo.yaml's (n_steps 64, batch_size 64, n_epochs 20, learning_rate 7e-5, net_arch [64, 64],
log_std_init -2.7, ortho_init false).  A demonstration of the plumbing; it carries no claim about learning curves.

With n_envs * n_steps rows per rollout, n_epochs 20 and batch_size 64 a rollout of 4096 envs is 81 920 minibatch steps: whether a run at thousands of envs
keeps the reference's batch size is the user's decision.

--seeds: the seeds of one cell as a population (ppo.PpoPopulation), --n-envs split into equal groups, one set of launches per minibatch step for all of them;
a JSON line then carries a list `members` with an entry per seed.

python tools/train_ppo.py --n-envs 256 --rollouts 10
python tools/train_ppo.py --n-envs 50 --rollouts 10 --seeds 0 1 2 3 4

--sweep NAME=v1,v2,... (repeatable; NAME one of learning_rate, clip_range, clip_range_vf, ent_coef, vf_coef, max_grad_norm; "none" is clip_range_vf's None) crosses
the values with each other and with --seeds (default: --seed alone) into one population, value-major and seed-minor.  Each entry of `members` then carries its
own values under `hyper`; the model folders hold member_<p>.npz and population.npz, which names what varies.

python tools/train_ppo.py --n-envs 60 --rollouts 10 --seeds 0 1 2 --sweep clip_range=0.1,0.2 --sweep ent_coef=0,0.01"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, '.')
import human_robot_gym_amd as hrg   # noqa: E402
from human_robot_gym_amd.ppo import MAX_POPULATION, PpoPopulation   # noqa: E402
from human_robot_gym_amd.training_utils import checked_sweep, member_lines, run_folder_from_args   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--env-id", default="ReachHuman")
ap.add_argument("--n-envs", type=int, default=256)
ap.add_argument("--horizon", type=int, default=100)
ap.add_argument("--n-steps", type=int, default=64)
ap.add_argument("--rollouts", type=int, default=10)
ap.add_argument("--batch-size", type=int, default=64)
ap.add_argument("--n-epochs", type=int, default=20)
ap.add_argument("--learning-rate", type=float, default=7e-5)
ap.add_argument("--gamma", type=float, default=0.99)
ap.add_argument("--gae-lambda", type=float, default=0.9)
ap.add_argument("--log-std-init", type=float, default=-2.7)
ap.add_argument("--separate", action="store_true", help="net_arch [dict(pi=[64, 64], vf=[64, 64])] instead of the shared [64, 64]")
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--seeds", type=int, nargs="+", default=None, help="a population: one member per seed, n-envs / len(seeds) envs each (the env itself is seeded with --seed)")
ap.add_argument("--sweep", action="append", default=None, metavar="NAME=v1,v2,...", help="a population over these values of a per-member hyper-parameter, crossed with "
                "further --sweep options and with --seeds (value-major, seed-minor); n-envs / members envs each")
ap.add_argument("--model-dir", default=None, help="models/<run_id>: checkpoints model_<step>.npz every --save-freq env steps and model_final.npz at the end")
ap.add_argument("--save-freq", type=int, default=0, help="env steps between checkpoints (with --model-dir)")
ap.add_argument("--eval-episodes", type=int, default=0, help="evaluate the deterministic policy on a second env after every block (n_test_episodes)")
ap.add_argument("--eval-n-envs", type=int, default=64)
ap.add_argument("--eval-seed", type=int, default=None, help="seed of the evaluation env (default: --seed + 1)")
ap.add_argument("--init-checkpoint", default=None, metavar="PATH", help="start from the parameters of this checkpoint (tools/pretrain_bc.py --out): the state_dict only, "
                "with fresh optimiser state and counters; a lone learner of the checkpoint's shapes")


def members_of(args):
    """(the members' seeds, the members' values of the swept fields) of --seeds and --sweep; ValueError before any env is built."""
    return checked_sweep(PpoPopulation, args.sweep, [args.seed] if args.seeds is None else args.seeds, args.n_envs, MAX_POPULATION)


def main(args):
    population = args.seeds is not None or args.sweep is not None
    if population and args.init_checkpoint is not None:
        raise NotImplementedError("--init-checkpoint with --seeds / --sweep: the checkpoint is a lone learner's")
    seeds, swept = members_of(args) if population else (None, {})
    env = hrg.HipVecEnv(args.n_envs, env_id=args.env_id, env_kwargs=dict(horizon=args.horizon, seed=args.seed))
    env.attach_rollout(n_steps=args.n_steps, gamma=args.gamma, gae_lambda=args.gae_lambda)
    kw = dict(batch_size=args.batch_size, n_epochs=args.n_epochs, learning_rate=args.learning_rate, log_std_init=args.log_std_init, ortho_init=False,
              net_arch=[dict(pi=[64, 64], vf=[64, 64])] if args.separate else [64, 64])
    if population:
        run_population(args, env, {**kw, **swept}, seeds, swept)
        env.close()
        return
    learner = env.attach_ppo(seed=args.seed, **kw)
    if args.init_checkpoint is not None:
        learner.load_parameters(args.init_checkpoint)
    run = run_folder_from_args(args)
    t0 = time.time()
    for k in range(args.rollouts):
        env.collect_rollout(learner.policy, learner.value)
        learner.train(env.rollout)
        line = dict(rollout=k, env_steps=(k + 1) * args.n_steps * args.n_envs, seconds=round(time.time() - t0, 3))
        line.update(env.rollout.episode_stats())
        line.update(learner.diagnostics())
        line.update(run.after(learner, line["env_steps"]))
        print(json.dumps(line), flush=True)
    run.finish(learner)
    env.close()


def run_population(args, env, kw, seeds, swept):
    """The loop of `main` for the members of --seeds and --sweep."""
    P = len(seeds)
    pop = env.attach_ppo_population(P, seeds=seeds, **kw)
    eval_env, first, saved_until = None, None, 0
    if args.eval_episodes > 0:
        eval_env = hrg.HipVecEnv(args.eval_n_envs, env_id=args.env_id, env_kwargs=dict(horizon=args.horizon, seed=args.seed + 1 if args.eval_seed is None else args.eval_seed))
        first = pop.member(0)   # (the shapes the stacked parameters follow)
    t0 = time.time()
    for k in range(args.rollouts):
        env.collect_rollout(pop.policy, pop.value)
        pop.train(env.rollout)
        env_steps = (k + 1) * args.n_steps * args.n_envs
        line = dict(rollout=k, env_steps=env_steps, seconds=round(time.time() - t0, 3))
        members = member_lines(pop.seeds, swept, env.rollout.episode_stats(groups=P), pop.diagnostics())
        if eval_env is not None:
            for m, res in zip(members, eval_env.evaluate(pop.p.params, args.eval_episodes, learner=first).by_policy()):
                m.update(eval_mean_reward=res.mean_reward, eval_std_reward=res.std_reward, eval_mean_ep_length=res.mean_ep_length)
        if args.model_dir is not None and args.save_freq > 0 and env_steps // args.save_freq > saved_until:
            saved_until = env_steps // args.save_freq
            line["checkpoint"] = pop.save(os.path.join(args.model_dir, f"model_{env_steps}"))
        line["members"] = members
        print(json.dumps(line), flush=True)
    if args.model_dir is not None:
        pop.save(os.path.join(args.model_dir, "model_final"))
    if first is not None:
        first.close()
        eval_env.close()


if __name__ == "__main__":   # (imported: the parser `ap` only)
    main(ap.parse_args())
