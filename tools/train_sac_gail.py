"""SAC on a discriminator's reward (adversarial.py, csrc/hrgym_disc.h), the whole alternation on one GPU: `env.collect_steps(learner.act,
train_freq)`, then `adversarial.train_sac(learner, env.replay, env.discriminator, gradient_steps, disc_every, alpha)`; uniform random actions until
`learning_starts` transitions are stored, as in tools/train_sac.py, whose shape this tool copies.  One JSON line per block: `env.replay.episode_stats()`,
`learner.diagnostics()` and, under `disc_`, `env.discriminator.diagnostics()`.  A demonstration of the plumbing; it carries no claim about learning curves.

python tools/create_expert_dataset.py --env ReachHuman --name reach-demo --episodes 200 --horizon 100
python tools/train_sac_gail.py --n-envs 1024 --dataset reach-demo --alpha 0.25 --gradient-steps 800 --blocks 5"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, '.')
import torch   # noqa: E402
import human_robot_gym_amd as hrg   # noqa: E402
from human_robot_gym_amd import adversarial   # noqa: E402
from human_robot_gym_amd.training_utils import run_folder_from_args   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--env-id", default="ReachHuman")
ap.add_argument("--dataset", required=True, help="a name (datasets/<name>/hrg_dataset.npz) or a path: the demonstrations the discriminator tells the learner's rows from")
ap.add_argument("--alpha", type=float, default=1.0, help="weight of the discriminator's reward against the env's: r_disc alpha + r_env (1 - alpha)")
ap.add_argument("--reward", choices=sorted(adversarial.REWARDS), default="gail", help="gail: -log(1 - D); airl: logit D")
ap.add_argument("--disc-every", type=int, default=1, help="gradient steps between two discriminator updates (0: never)")
ap.add_argument("--disc-lr", type=float, default=3e-4)
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
ap.add_argument("--model-dir", default=None, help="models/<run_id>: checkpoints model_<step>.npz every --save-freq env steps and model_final.npz at the end, the "
                "discriminator's state_dict next to each as disc_<step>.pt")
ap.add_argument("--save-freq", type=int, default=0, help="env steps between checkpoints (with --model-dir)")
ap.add_argument("--eval-episodes", type=int, default=0, help="evaluate the deterministic policy on a second env before the first and after every block (the env's own reward)")
ap.add_argument("--eval-n-envs", type=int, default=64)
ap.add_argument("--eval-seed", type=int, default=None, help="seed of the evaluation env (default: --seed + 1)")


def save_disc(disc, checkpoint):
    """The discriminator's state_dict next to the learner's checkpoint model_<step>.npz, as disc_<step>.pt."""
    folder, name = os.path.split(checkpoint)
    path = os.path.join(folder, "disc_" + name[len("model_"):].rsplit(".", 1)[0] + ".pt")
    torch.save(disc.state_dict(), path)
    return path


def main(args):
    env = hrg.HipVecEnv(args.n_envs, env_id=args.env_id, env_kwargs=dict(horizon=args.horizon, seed=args.seed))
    env.attach_replay(args.buffer_size)
    learner = env.attach_sac(batch_size=args.batch_size, learning_rate=args.learning_rate, ent_coef=args.ent_coef, seed=args.seed)
    disc = env.attach_discriminator(args.dataset, batch_size=args.batch_size, learning_rate=args.disc_lr, reward=args.reward, seed=args.seed)
    gen = torch.Generator(device=learner.device).manual_seed(args.seed)

    def uniform(obs):
        return torch.rand(obs.shape[0], learner.act_dim, generator=gen, device=obs.device) * 2.0 - 1.0

    run = run_folder_from_args(args)
    if run.eval_env is not None:
        res = run.eval_env.evaluate(learner, args.eval_episodes)
        print(json.dumps(dict(block=-1, env_steps=0, table_rows=disc.table.n_rows, eval_mean_reward=res.mean_reward, eval_std_reward=res.std_reward,
                              eval_mean_ep_length=res.mean_ep_length)), flush=True)
    t0 = time.time()
    for block in range(args.blocks):
        warm = env.replay.size() * args.n_envs < args.learning_starts
        env.collect_steps(uniform if warm else learner.act, args.train_freq)
        if env.replay.size() * args.n_envs >= args.learning_starts:
            adversarial.train_sac(learner, env.replay, disc, args.gradient_steps, disc_every=args.disc_every, alpha=args.alpha)
        line = dict(block=block, env_steps=(block + 1) * args.train_freq * args.n_envs, policy="uniform" if warm else "actor", seconds=round(time.time() - t0, 3))
        line.update(env.replay.episode_stats())
        if learner.n_updates:
            line.update(learner.diagnostics())
        if disc.n_updates:
            line.update({"disc_" + k: v for k, v in disc.diagnostics().items()})
        line.update(run.after(learner, line["env_steps"]))
        if "checkpoint" in line:
            line["disc_checkpoint"] = save_disc(disc, line["checkpoint"])
        print(json.dumps(line), flush=True)
    final = run.finish(learner)
    if final is not None:
        save_disc(disc, final)
    env.close()


if __name__ == "__main__":   # (imported: the parser `ap` only)
    main(ap.parse_args())
