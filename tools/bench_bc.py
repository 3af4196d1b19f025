"""What one behaviour-cloning step costs on the device (csrc/hrgym_bc.h), written to profiles/r31_bc.json: milliseconds per bc step -- two
launches, the rows drawn from the table by the handle -- at ReachHuman's shapes: observations of 18 values, 7 actions, net_arch [64, 64, 64], a table of
100 000 rows, batches of 128 and 256, for a SAC actor and a PPO actor.  After tools/bench_sac.py, whose whole SAC step (replay.sample + six launches) is the
figure to read it beside: run both in one session.

Warm-up block first; then blocks of `--steps` steps, HIP events around each block, no synchronisation inside a block.
python tools/bench_bc.py [--blocks 7] [--steps 200]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, '.')
import torch   # noqa: E402
from human_robot_gym_amd.bc import BehaviourCloning, DemoTable   # noqa: E402
from human_robot_gym_amd.ppo import PpoLearner   # noqa: E402
from human_robot_gym_amd.sac import SacLearner   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--rows", type=int, default=100_000, help="rows of the table")
ap.add_argument("--batch-sizes", type=int, nargs="+", default=[128, 256])
ap.add_argument("--out", default="profiles/r31_bc.json")
K, A, ARCH, LR = 18, 7, [64, 64, 64], 1e-3


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main(args):
    out = dict(obs_dim=K, act_dim=A, net_arch=ARCH, table_rows=args.rows, steps_per_block=args.steps, blocks=args.blocks, device=torch.cuda.get_device_name(0))
    g = torch.Generator().manual_seed(0)
    obs, act = torch.randn(args.rows, K, generator=g).cuda(), (torch.rand(args.rows, A, generator=g) * 2.0 - 1.0).cuda()
    for kind in ("sac", "ppo"):
        for B in args.batch_sizes:
            learner = SacLearner(K, A, net_arch=ARCH, batch_size=128, seed=0) if kind == "sac" else PpoLearner(K, A, net_arch=ARCH, batch_size=128, seed=0)
            bc = BehaviourCloning(learner, DemoTable(obs, act, kind), batch_size=B, learning_rate=LR, seed=0)
            bc.train(args.steps)   # warm-up
            first = bc.diagnostics()["loss"]
            ms = [timed(lambda: bc.train(args.steps)) / args.steps for _ in range(args.blocks)]
            med, diag = float(np.median(ms)), bc.diagnostics()
            out[f"{kind}_batch_{B}"] = dict(kind=kind, batch_size=B, ms_per_step=ms, ms_median=med, ms_spread=float(np.max(ms) - np.min(ms)), entries_updated=bc.n_entries,
                                            loss_after_warm_up=first, loss=diag["loss"], n_updates=diag["n_updates"], finite=bool(torch.isfinite(learner.p.params).all()))
            print("%s, batch %3d: %.4f ms per bc step (the draws included; blocks %s)" % (kind, B, med, " ".join("%.4f" % x for x in ms)))
            bc.close()
            learner.close()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":   # (imported: the parser `ap` only)
    main(ap.parse_args())
