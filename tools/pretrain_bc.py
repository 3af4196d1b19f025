#!/usr/bin/env python3
"""Pre-train an actor on a demonstration dataset by behaviour cloning on the device (bc.BehaviourCloning; csrc/hrgym_bc.h), and write the
learner's checkpoint, which tools/train_sac.py / tools/train_ppo.py --init-checkpoint and tools/evaluate.py read:

  python tools/create_expert_dataset.py --env ReachHuman --name reach-demo --episodes 100
  python tools/pretrain_bc.py --env ReachHuman --dataset reach-demo --algorithm sac --steps 2000 --eval-episodes 20 --out models/reach-bc/model_final.npz

The env is built as tools/create_expert_dataset.py builds it for that task (the task's env_kwargs and clips, the IK front-end for the Cartesian tasks, and its
--shield, --geometry, --done-at-success, --action-limit, --horizon: pass what the dataset was recorded with; another task, action form or geometry is refused), with the
replay buffer (sac) or the rollout buffer (ppo) attached: the table holds that buffer's view of the dataset's rows.  One JSON line: the mean squared error on the
first batch and on the last, the steps, and with --eval-episodes the deterministic policy's evaluation before and after.  SAC's critics are not pre-trained: the
first SAC updates after loading the checkpoint follow random critics, which is why the evaluation here is reported before and after."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--env", required=True)
ap.add_argument("--dataset", required=True, help="dataset_name (datasets/<name>/hrg_dataset.npz) or a path")
ap.add_argument("--algorithm", choices=["sac", "ppo"], default="sac")
ap.add_argument("--steps", type=int, default=1000, help="behaviour-cloning steps")
ap.add_argument("--batch-size", type=int, default=128)
ap.add_argument("--learning-rate", type=float, default=1e-3)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--eval-episodes", type=int, default=0, help="evaluate the deterministic policy before and after (env.evaluate)")
ap.add_argument("--depth", type=int, default=None, help="hidden layers of width 64 (default: 3 for sac, 2 for ppo, the training tools')")
ap.add_argument("--separate", action="store_true", help="ppo: net_arch [dict(pi=..., vf=...)] instead of the shared trunk")
ap.add_argument("--log-std-init", type=float, default=-2.7, help="ppo")
ap.add_argument("--n-envs", type=int, default=64, help="envs of the evaluation")
ap.add_argument("--horizon", type=int, default=None)
ap.add_argument("--shield", default="SSM")
ap.add_argument("--geometry", default="capsule", help="robot_geometry, capsule | hull: the one the dataset was recorded with (another is refused)")
ap.add_argument("--done-at-success", choices=["true", "false"], default=None, help="environment.done_at_success of the evaluations (default: the task's)")
ap.add_argument("--action-limit", type=float, default=0.1, help="ik_position_delta.action_limit of the Cartesian tasks")
ap.add_argument("--out", required=True, help="the learner's checkpoint (.npz)")


def main(args):
    import human_robot_gym_amd as hrg
    from human_robot_gym_amd.mixed import task_clips, task_env_kwargs
    kw = dict(shield_type=args.shield, seed=args.seed, **task_env_kwargs(args.env))
    if args.horizon is not None:
        kw["horizon"] = args.horizon
    if args.done_at_success is not None:
        kw["done_at_success"] = args.done_at_success == "true"
    env = hrg.HipVecEnv(args.n_envs, env_id=args.env, env_kwargs=kw, clips=task_clips(args.env), robot_geometry=args.geometry,
                        ik_position_delta=None if args.env == "ReachHuman" else dict(action_limit=args.action_limit))
    if args.algorithm == "sac":   # the shapes tools/train_sac.py and tools/train_ppo.py build, so that --init-checkpoint fits
        env.attach_replay(args.n_envs)
        learner = env.attach_sac(net_arch=[64] * (args.depth or 3), seed=args.seed)
    else:
        layers = [64] * (args.depth or 2)
        env.attach_rollout(n_steps=32)
        learner = env.attach_ppo(batch_size=32, net_arch=[dict(pi=layers, vf=list(layers))] if args.separate else layers, log_std_init=args.log_std_init, ortho_init=False,
                                 seed=args.seed)
    table = env.demonstrations(args.dataset)
    bc = env.attach_bc(table, batch_size=args.batch_size, learning_rate=args.learning_rate, seed=args.seed)
    line = dict(env=args.env, dataset=args.dataset, algorithm=args.algorithm, rows=table.n_rows, steps=args.steps, batch_size=args.batch_size, learning_rate=args.learning_rate)

    def evaluate(when):
        if args.eval_episodes > 0:
            res = env.evaluate(learner, args.eval_episodes)
            line.update({f"eval_mean_reward_{when}": res.mean_reward, f"eval_std_reward_{when}": res.std_reward, f"eval_mean_ep_length_{when}": res.mean_ep_length})

    evaluate("before")
    if args.steps > 0:
        bc.step()
        line["loss_before"] = bc.diagnostics()["loss"]   # the error of the untrained actor on the first batch
        bc.train(args.steps - 1)
        line["loss_after"] = bc.diagnostics()["loss"]
    evaluate("after")
    line["checkpoint"] = learner.save(args.out)
    print(json.dumps(line), flush=True)
    env.close()


if __name__ == "__main__":   # (imported: the parser `ap` only)
    main(ap.parse_args())
