#!/usr/bin/env python3
"""DAgger on the device (dagger.Dagger; csrc/hrgym_dagger.h): iterations of (collect with the mixture of the learner and the live scripted expert,
every visited row labelled by the expert; behaviour cloning on the aggregated table), and the learner's checkpoint, which tools/train_sac.py / tools/train_ppo.py
--init-checkpoint and tools/evaluate.py read:

  python tools/train_dagger.py --env ReachHuman --algorithm sac --iterations 10 --collect-steps 100 --bc-steps 500 --eval-episodes 20 --out models/reach-dagger/model_final.npz
  python tools/train_dagger.py --env ReachHuman --seed-dataset reach-demo --beta0 1 --decay 0 --critic-steps 200 --out ...    # iteration 0: the expert drives, the replay
                                                                                                                               # buffer fills with its transitions

Iteration i collects with beta_i = beta0 * decay^i (the probability that the expert drives an env's step).  The env is built as tools/create_expert_dataset.py builds
it for that task, with the task's scripted expert at signal_to_noise_ratio --snr (1: clean labels; every collected step advances the expert's noise once).
--seed-dataset: a demonstration dataset whose rows are the head of the table and are never overwritten.  --critic-steps (sac): SAC updates on the replay buffer
after each collection, which holds the mixture's transitions with their rewards.  One JSON line per iteration: beta, env.dagger.stats() (steps, the share the expert
drove, the on-policy imitation error), the behaviour-cloning loss, and with --eval-episodes the deterministic policy's evaluation."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--env", required=True)
ap.add_argument("--algorithm", choices=["sac", "ppo"], default="sac")
ap.add_argument("--iterations", type=int, default=10)
ap.add_argument("--collect-steps", type=int, default=100, help="env steps per iteration (of every env)")
ap.add_argument("--bc-steps", type=int, default=500, help="behaviour-cloning steps per iteration")
ap.add_argument("--beta0", type=float, default=0.5)
ap.add_argument("--decay", type=float, default=0.7)
ap.add_argument("--capacity", type=int, default=1_000_000, help="transitions the table holds behind the seed dataset's rows; the oldest step is overwritten")
ap.add_argument("--seed-dataset", default=None, help="dataset_name (datasets/<name>/hrg_dataset.npz) or a path: the pinned head of the table")
ap.add_argument("--critic-steps", type=int, default=0, help="sac: learner.train(env.replay, k) after each collection")
ap.add_argument("--buffer-size", type=int, default=1_000_000, help="sac: the replay buffer")
ap.add_argument("--batch-size", type=int, default=128)
ap.add_argument("--learning-rate", type=float, default=1e-3)
ap.add_argument("--snr", type=float, default=1.0, help="signal_to_noise_ratio of the expert")
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--eval-episodes", type=int, default=0, help="evaluate the deterministic policy after each iteration (env.evaluate)")
ap.add_argument("--depth", type=int, default=None, help="hidden layers of width 64 (default: 3 for sac, 2 for ppo, the training tools')")
ap.add_argument("--separate", action="store_true", help="ppo: net_arch [dict(pi=..., vf=...)] instead of the shared trunk")
ap.add_argument("--log-std-init", type=float, default=-2.7, help="ppo")
ap.add_argument("--n-envs", type=int, default=64)
ap.add_argument("--horizon", type=int, default=None)
ap.add_argument("--shield", default="SSM")
ap.add_argument("--geometry", default="capsule", help="robot_geometry, capsule | hull")
ap.add_argument("--done-at-success", choices=["true", "false"], default=None, help="environment.done_at_success (default: the task's)")
ap.add_argument("--action-limit", type=float, default=0.1, help="ik_position_delta.action_limit of the Cartesian tasks")
ap.add_argument("--out", required=True, help="the learner's checkpoint (.npz)")


def beta_of(args, i):
    return args.beta0 * args.decay ** i


def main(args):
    import human_robot_gym_amd as hrg
    from human_robot_gym_amd.expert import EXPERT_ENVS
    from human_robot_gym_amd.mixed import task_clips, task_env_kwargs
    eid = next((k for k, envs in EXPERT_ENVS.items() if args.env in envs), None)
    if eid is None:
        sys.exit(f"--env {args.env}: no scripted expert reads this task's observation ({sorted(e for v in EXPERT_ENVS.values() for e in v)})")
    kw = dict(shield_type=args.shield, seed=args.seed, **task_env_kwargs(args.env))
    if args.horizon is not None:
        kw["horizon"] = args.horizon
    if args.done_at_success is not None:
        kw["done_at_success"] = args.done_at_success == "true"
    env = hrg.HipVecEnv(args.n_envs, env_id=args.env, env_kwargs=kw, clips=task_clips(args.env), robot_geometry=args.geometry,
                        expert=dict(id=eid, signal_to_noise_ratio=args.snr, seed=args.seed),
                        ik_position_delta=None if args.env == "ReachHuman" else dict(action_limit=args.action_limit))
    if args.algorithm == "sac":   # the shapes tools/train_sac.py and tools/train_ppo.py build, so that --init-checkpoint fits
        env.attach_replay(args.buffer_size)
        learner = env.attach_sac(net_arch=[64] * (args.depth or 3), batch_size=args.batch_size, seed=args.seed)
    else:
        layers = [64] * (args.depth or 2)
        env.attach_rollout(n_steps=32)
        learner = env.attach_ppo(batch_size=32, net_arch=[dict(pi=layers, vf=list(layers))] if args.separate else layers, log_std_init=args.log_std_init, ortho_init=False,
                                 seed=args.seed)
    dagger = env.attach_dagger(args.capacity, beta=args.beta0, table=None if args.seed_dataset is None else env.demonstrations(args.seed_dataset), seed=args.seed)
    bc = env.attach_bc(dagger.table, batch_size=args.batch_size, learning_rate=args.learning_rate, seed=args.seed)
    for i in range(args.iterations):
        dagger.beta = beta_of(args, i)
        env.collect_dagger(args.collect_steps)
        line = dict(iteration=i, **dagger.stats())
        if args.algorithm == "sac" and args.critic_steps > 0:
            learner.train(env.replay, args.critic_steps)
        bc.train(args.bc_steps)
        if args.bc_steps > 0:
            line["bc_loss"] = bc.diagnostics()["loss"]
        if args.eval_episodes > 0:
            res = env.evaluate(learner, args.eval_episodes)
            line.update(eval_mean_reward=res.mean_reward, eval_std_reward=res.std_reward, eval_mean_ep_length=res.mean_ep_length)
        print(json.dumps(line), flush=True)
    print(json.dumps(dict(checkpoint=learner.save(args.out))), flush=True)
    env.close()


if __name__ == "__main__":   # (imported: the parser `ap` and beta_of only)
    main(ap.parse_args())
