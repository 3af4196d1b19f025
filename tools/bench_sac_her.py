"""What one SAC + HER gradient step costs on the device, sampling included, written to profiles/r15_sac_her.json: milliseconds per (sample, gradient step) at the
shape of training/config/algorithm/sac_her.yaml -- batch 128, net_arch [64, 64, 64], 7 actions, a ReachHuman feature row of 6 + 6 + 18 values -- and at batch
256, out of a hindsight buffer at a user's size: 1024 envs, horizon 100, full rings of 200 slots.

Two ways to the same step, both reading the same buffer:
  composed  what the code offered before the fused sampler: `her.sample(B)` (nine outputs, a prefix sum and a read of its total per call: one stream
            synchronisation), two `torch.cat` over the dict entries, `SacLearner.step`;
  train     `learner.train(her, steps)`: one read of the buffer's size, then `her.sample_features(B)` and `step` with nothing synchronising.
Warm-up block first; then `--blocks` blocks of `--steps` gradient steps per side, alternating between the sides in one process, HIP events around each block.
The buffer's content is synthetic (random rows, staggered time limits): the cost of a step does not depend on the values.
python tools/bench_sac_her.py [--blocks 7] [--steps 128] [--out profiles/r15_sac_her.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, '.')
import torch   # noqa: E402
from human_robot_gym_amd._cstruct import CONST   # noqa: E402
from human_robot_gym_amd.her import HerBuffer, build_her_desc   # noqa: E402
from human_robot_gym_amd.replay import ReplayBufferSamples   # noqa: E402
from human_robot_gym_amd.sac import SacLearner   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--steps", type=int, default=128, help="gradient steps per block")
ap.add_argument("--out", default="profiles/r15_sac_her.json")
args = ap.parse_args()
A, ARCH, LR, n_envs, horizon, cap = 7, [64, 64, 64], 5e-4, 1024, 100, 200
OBS_COLS = list(range(0, 12)) + list(range(18, 24))   # object-state, robot0_joint_pos: 18 values


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


her = HerBuffer(build_her_desc(n_envs, cap, horizon, "reach", OBS_COLS, act_dim=A, n_sampled_goal=4, goal_selection_strategy="future", seed=1, goal_dist=0.5))
gen = torch.Generator(device="cuda").manual_seed(0)
rows = lambda: torch.rand(n_envs, CONST["HRG_OBS_DIM"], generator=gen, device="cuda") * 2.0 - 1.0   # noqa: E731
her.observe(rows())
env_ix = torch.arange(n_envs, device="cuda")
info = torch.zeros(n_envs, CONST["HRG_INFO_DIM"], dtype=torch.int32, device="cuda")
for t in range(3 * horizon):   # env e's time limit falls on the steps with (t + e) % horizon == horizon - 1: after the first, every episode is `horizon` steps long
    done = ((t + env_ix) % horizon == horizon - 1).to(torch.uint8)
    info[:, CONST["HRG_INFO_TRUNCATED"]] = done.to(torch.int32)
    her.add_step((torch.rand(n_envs, CONST["HRG_ACT_DIM"], generator=gen, device="cuda") * 2.0 - 1.0).double(), rows(), rows(),
                 torch.rand(n_envs, generator=gen, device="cuda") - 1.0, done, info)
stored, closed, _ = her.counts_host()
F = her.obs_features
out = dict(net_arch=ARCH, act_dim=A, obs_features=F, n_envs=n_envs, horizon=horizon, capacity=cap, stored=stored, sampleable=closed, blocks=args.blocks,
           steps_per_block=args.steps, device=torch.cuda.get_device_name(0), cases=[])
cat = lambda d: torch.cat([d["achieved_goal"], d["desired_goal"], d["observation"]], dim=1)   # noqa: E731
for B in (128, 256):
    learners = {side: SacLearner(F, A, net_arch=ARCH, learning_rate=LR, ent_coef="auto_0.2", batch_size=B, seed=0) for side in ("composed", "train")}

    def composed_block():
        learner = learners["composed"]
        for _ in range(args.steps):
            d = her.sample(B)
            learner.step(ReplayBufferSamples(cat(d.observations), d.actions, cat(d.next_observations), d.dones, d.rewards))

    def train_block():
        learners["train"].train(her, args.steps)

    sides = (("composed", composed_block), ("train", train_block))
    for _, fn in sides:   # warm-up: every kernel and shape of the timed windows
        fn()
    ms = {side: [] for side, _ in sides}
    for _ in range(args.blocks):
        for side, fn in sides:
            ms[side].append(timed(fn) / args.steps)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: float(np.max(v) - np.min(v)) for k, v in ms.items()}
    res = dict(batch_size=B, composed_ms_per_step=ms["composed"], train_ms_per_step=ms["train"], composed_ms_median=med["composed"], train_ms_median=med["train"],
               composed_ms_spread=spread["composed"], train_ms_spread=spread["train"], composed_over_train=med["composed"] / med["train"],
               train_not_above_composed_by_more_than_the_larger_spread=bool(med["train"] <= med["composed"] + max(spread.values())),
               finite=bool(all(torch.isfinite(v).all() for l in learners.values() for v in l.state_dict().values())),
               n_updates={k: l.n_updates for k, l in learners.items()})
    print("batch %3d: composed (sample, 2 x cat, step) %.4f ms per gradient step (blocks %s), train (sample_features, step) %.4f ms (blocks %s): %.2f x"
          % (B, med["composed"], " ".join("%.4f" % x for x in ms["composed"]), med["train"], " ".join("%.4f" % x for x in ms["train"]), res["composed_over_train"]), flush=True)
    out["cases"].append(res)
    for l in learners.values():
        l.close()
her.close()
os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
