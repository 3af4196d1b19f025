"""What adversarial imitation adds to a SAC gradient step on the device (csrc/hrgym_disc.h), written to profiles/r33_disc.json: milliseconds, at
tools/bench_sac.py's shapes (batch 128, observations of 18 values, 4 actions, net_arch [64, 64, 64], a table of 100 000 rows), of
  disc_step    one discriminator update (two launches; the expert rows drawn from the table by the handle, the policy rows a fixed batch),
  reward       one reward call on n = 128 rows (one launch, the env's rewards mixed in place),
  train_sac    the whole adversarial.train_sac gradient step (replay.sample, discriminator update, reward, the six launches of the SAC step),
  sac_train    learner.train's gradient step (replay.sample, the six launches) beside it: the figure of profiles/r31_sac.json, measured again here.
All four in one process, alternating block by block.  Warm-up block first; then blocks of `--steps` iterations, HIP events around each block, no
synchronisation inside a block.
python tools/bench_gail.py [--blocks 7] [--steps 200]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, '.')
import torch   # noqa: E402
from human_robot_gym_amd import adversarial   # noqa: E402
from human_robot_gym_amd._cstruct import CONST   # noqa: E402
from human_robot_gym_amd.bc import DemoTable   # noqa: E402
from human_robot_gym_amd.replay import ReplayBuffer, build_replay_desc   # noqa: E402
from human_robot_gym_amd.sac import SacLearner   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--rows", type=int, default=100_000, help="rows of the table")
ap.add_argument("--out", default="profiles/r33_disc.json")
B, K, A, ARCH, LR, n_envs, slots = 128, 18, 4, [64, 64, 64], 5e-4, 64, 16


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def full_buffer(rng):
    """A replay buffer of `n_envs` envs with every slot filled (tools/bench_sac.py's)."""
    rb = ReplayBuffer(build_replay_desc(n_envs, n_envs * slots, list(range(K)), act_dim=A, seed=1))
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()   # noqa: E731
    rb.observe(dev(rng.uniform(-1, 1, (n_envs, 64))))
    for _ in range(slots):
        rb.add_step(dev(rng.uniform(-1, 1, (n_envs, A))), dev(rng.uniform(-1, 1, (n_envs, 64))), dev(rng.uniform(-1, 1, (n_envs, 64))), dev(rng.normal(size=n_envs)),
                    torch.from_numpy((rng.uniform(size=n_envs) < 0.05).astype(np.uint8)).cuda(), torch.zeros(n_envs, CONST["HRG_INFO_DIM"], dtype=torch.int32).cuda())
    return rb


def main(args):
    out = dict(batch_size=B, obs_dim=K, act_dim=A, net_arch=ARCH, table_rows=args.rows, steps_per_block=args.steps, blocks=args.blocks, device=torch.cuda.get_device_name(0))
    rb = full_buffer(np.random.RandomState(0))
    g = torch.Generator().manual_seed(0)
    table = DemoTable(torch.randn(args.rows, K, generator=g).cuda(), (torch.rand(args.rows, A, generator=g) * 2.0 - 1.0).cuda(), "sac")
    # two learners and two discriminators, so that each timed loop continues its own run
    plain, mixed = (SacLearner(K, A, net_arch=ARCH, learning_rate=LR, ent_coef="auto_0.2", batch_size=B, seed=0) for _ in range(2))
    alone, inside = (adversarial.Discriminator(table, net_arch=ARCH, batch_size=B, learning_rate=3e-4, seed=0) for _ in range(2))
    batch = rb.sample(B)
    rewards = batch.rewards.clone()

    def disc_block():
        for _ in range(args.steps):
            alone.step(batch.observations, batch.actions)

    def reward_block():
        for _ in range(args.steps):
            alone.reward(batch.observations, batch.actions, env_rewards=rewards, alpha=0.25, out=rewards)

    blocks = dict(disc_step=disc_block, reward=reward_block, train_sac=lambda: adversarial.train_sac(mixed, rb, inside, args.steps, disc_every=1, alpha=0.25),
                  sac_train=lambda: plain.train(rb, args.steps))
    for fn in blocks.values():   # warm-up: every kernel and shape of the timed windows
        fn()
    ms = {k: [] for k in blocks}
    for _ in range(args.blocks):
        for key, fn in blocks.items():
            ms[key].append(timed(fn) / args.steps)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    for k in blocks:
        out[k] = dict(ms_per_step=ms[k], ms_median=med[k], ms_spread=float(np.max(ms[k]) - np.min(ms[k])))
        print("%-10s %.4f ms (blocks %s)" % (k, med[k], " ".join("%.4f" % x for x in ms[k])))
    out["train_sac_over_sac_train"] = med["train_sac"] / med["sac_train"]
    out["diagnostics"] = inside.diagnostics()
    out["finite"] = bool(torch.isfinite(mixed.p.params).all() and torch.isfinite(inside.p.params).all() and torch.isfinite(alone.p.params).all())
    print("train_sac / sac_train = %.3f; n_updates %d, finite %s" % (out["train_sac_over_sac_train"], inside.n_updates, out["finite"]))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for h in (alone, inside, plain, mixed, rb):
        h.close()


if __name__ == "__main__":   # (imported: the parser `ap` only)
    main(ap.parse_args())
