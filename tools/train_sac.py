"""The whole SAC alternation on one GPU, nothing leaving the device between the blocks: `env.collect_steps(learner.act, train_freq)`, then
`learner.train(env.replay, gradient_steps)`; uniform random actions until `learning_starts` transitions are stored (SB3's warm-up).  One JSON line per block:
`env.replay.episode_stats()` and `learner.diagnostics()`.  A demonstration of the plumbing; it carries no claim about learning curves.

--gradient-steps is explicit.  The ICRA configs say `train_freq: [100, step]`, `gradient_steps: -1`: in SB3 1.5.0 -1 means "as many gradient steps as
transitions were collected in the rollout", train_freq * n_envs.  With 8 envs that is 800 per block; with 4096 it would be 409 600: whether a run at thousands of
envs keeps that ratio is the user's decision.

python tools/train_sac.py --n-envs 1024 --gradient-steps 800 --blocks 20

--seeds 0 1 2 3 4 trains the five seeds of one cell of a study side by side as a population (sac.SacPopulation): the envs are five groups of n-envs / 5, member p
acts in and learns from group p only and equals, bit for bit, the lone run of its seed on its group's transitions.  --learning-starts then counts a member's
transitions; the JSON line carries `members`, one dict of episode stats and diagnostics per member; --model-dir receives model_<step>/member_<p>.npz.

python tools/train_sac.py --n-envs 1280 --seeds 0 1 2 3 4 --gradient-steps 800 --blocks 5

--sweep NAME=v1,v2,... (repeatable; NAME one of learning_rate, gamma, tau, ent_coef, target_entropy) crosses the values with each other and with --seeds (default:
--seed alone) into one population, value-major and seed-minor: a sweep of V values x S seeds costs what V S seeds cost.  Each entry of `members` then carries its
own values under `hyper`; the model folders hold member_<p>.npz and population.npz, which names what varies.

python tools/train_sac.py --n-envs 1536 --seeds 0 1 2 --sweep learning_rate=1e-3,3e-4 --sweep ent_coef=auto_0.2,0.1 --gradient-steps 800 --blocks 5"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, '.')
import torch   # noqa: E402
import human_robot_gym_amd as hrg   # noqa: E402
from human_robot_gym_amd.sac import MAX_POPULATION, SacPopulation   # noqa: E402
from human_robot_gym_amd.training_utils import checked_sweep, member_lines, run_folder_from_args   # noqa: E402

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
    return checked_sweep(SacPopulation, args.sweep, [args.seed] if args.seeds is None else args.seeds, args.n_envs, MAX_POPULATION)


def main(args):
    population = args.seeds is not None or args.sweep is not None
    if population and args.init_checkpoint is not None:
        raise NotImplementedError("--init-checkpoint with --seeds / --sweep: the checkpoint is a lone learner's")
    seeds, swept = members_of(args) if population else (None, {})
    env = hrg.HipVecEnv(args.n_envs, env_id=args.env_id, env_kwargs=dict(horizon=args.horizon, seed=args.seed))
    env.attach_replay(args.buffer_size)

    def run_population():
        """The loop below for the members of --seeds."""
        P = len(seeds)
        pop = env.attach_sac_population(P, seeds=seeds, **{**dict(batch_size=args.batch_size, learning_rate=args.learning_rate, ent_coef=args.ent_coef), **swept})
        gen = torch.Generator(device=pop.device).manual_seed(args.seed)
        uniform = lambda obs: torch.rand(obs.shape[0], pop.act_dim, generator=gen, device=obs.device) * 2.0 - 1.0   # noqa: E731
        eval_env, first, saved_until = None, None, 0
        if args.eval_episodes > 0:
            eval_env = hrg.HipVecEnv(args.eval_n_envs, env_id=args.env_id, env_kwargs=dict(horizon=args.horizon, seed=args.seed + 1 if args.eval_seed is None else args.eval_seed))
            first = pop.member(0)   # (the shapes the stacked parameters follow)
        per_member = args.n_envs // P
        t0 = time.time()
        for block in range(args.blocks):
            warm = env.replay.size() * per_member < args.learning_starts
            env.collect_steps(uniform if warm else pop.act, args.train_freq)
            if env.replay.size() * per_member >= args.learning_starts:
                pop.train(env.replay, args.gradient_steps)
            env_steps = (block + 1) * args.train_freq * args.n_envs
            line = dict(block=block, env_steps=env_steps, policy="uniform" if warm else "actor", seconds=round(time.time() - t0, 3))
            members = member_lines(pop.seeds, swept, env.replay.episode_stats(groups=P), *([pop.diagnostics()] if pop.n_updates else []))
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

    if population:
        run_population()
        env.close()
        return
    learner = env.attach_sac(batch_size=args.batch_size, learning_rate=args.learning_rate, ent_coef=args.ent_coef, seed=args.seed)
    if args.init_checkpoint is not None:
        learner.load_parameters(args.init_checkpoint)
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


if __name__ == "__main__":   # (imported: the parser `ap` only)
    main(ap.parse_args())
