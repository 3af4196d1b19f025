"""What the DAgger step adds to a collection step on the device (csrc/hrgym_dagger.h), written to profiles/r32_dagger.json: milliseconds per env
step of `env.collect_dagger(k)` with beta = 0 -- the learner drives every env, so the envs execute the rows collect_steps sends -- against
`env.collect_steps(lambda o: learner.act(o, deterministic=True), k)`, which is unchanged code: ReachHuman with the SSM shield, `--n-envs` envs, a SAC learner
[64, 64, 64] on the replay buffer, the ReachHuman expert at signal_to_noise_ratio 1.  What differs per step: collect_dagger launches the expert kernel and the dagger
kernel, which also writes the table's rows, where collect_steps launches the torch kernels that unscale and widen the action.

Both loops run in one process on one env, alternating: a warm-up block of each, then `--blocks` pairs of blocks of `--steps` steps, HIP events around each block,
no synchronisation inside a block.  The step kernel's time depends on where the envs are in their episodes (all of them reset together), so a block is one whole
episode of every env -- the horizon is `--steps` -- and the order within a pair alternates: neither loop always sees the same half of an episode.
python tools/bench_dagger.py [--n-envs 1024] [--blocks 8] [--steps 100]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--n-envs", type=int, default=1024)
ap.add_argument("--blocks", type=int, default=8, help="pairs of blocks")
ap.add_argument("--steps", type=int, default=100, help="steps of a block, and the horizon")
ap.add_argument("--out", default="profiles/r32_dagger.json")


def main(args):
    import torch
    import human_robot_gym_amd as hrg

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    n, k = args.n_envs, args.steps
    env = hrg.HipVecEnv(n, env_id="ReachHuman", env_kwargs=dict(shield_type="SSM", seed=0, horizon=k), clips=hrg.synthetic_clips(13, seed=0),
                        expert=dict(id="ReachHuman", signal_to_noise_ratio=1.0, seed=0))
    env.attach_replay(n * 4 * k)
    learner = env.attach_sac(net_arch=[64, 64, 64], batch_size=128, seed=0)
    dagger = env.attach_dagger(n * 4 * k, beta=0.0)
    loops = dict(collect_steps=lambda: env.collect_steps(lambda o: learner.act(o, deterministic=True), k), collect_dagger=lambda: env.collect_dagger(k))
    for fn in loops.values():   # warm-up: every kernel of both loops has run
        fn()
    ms = {name: [] for name in loops}
    for pair in range(args.blocks):
        for name in (list(loops) if pair % 2 == 0 else list(loops)[::-1]):
            ms[name].append(timed(loops[name]) / k)
    stats = dagger.stats()
    out = dict(env="ReachHuman", shield="SSM", n_envs=n, obs_dim=env.replay.obs_dim, act_dim=env.replay.act_dim, net_arch=[64, 64, 64], horizon=k, steps_per_block=k, blocks=args.blocks,
               device=torch.cuda.get_device_name(0), beta=0.0, expert_steps=stats["expert_steps"], table_rows=dagger.table.n_rows)
    for name, xs in ms.items():
        out[name] = dict(ms_per_step=xs, ms_median=float(np.median(xs)), ms_spread=float(np.max(xs) - np.min(xs)))
        print("%-15s %.4f ms per env step of %d envs (blocks %s)" % (name, out[name]["ms_median"], n, " ".join("%.4f" % x for x in xs)))
    out["ratio_of_medians"] = out["collect_dagger"]["ms_median"] / out["collect_steps"]["ms_median"]
    out["added_ms_per_step"] = out["collect_dagger"]["ms_median"] - out["collect_steps"]["ms_median"]
    print("collect_dagger / collect_steps = %.4f (+%.4f ms per step)" % (out["ratio_of_medians"], out["added_ms_per_step"]))
    env.close()
    path = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":   # (imported: the parser `ap` only)
    main(ap.parse_args())
