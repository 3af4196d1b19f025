"""What one PPO minibatch step costs on the device (csrc/hrgym_ppo.h), written to profiles/r14_ppo.json: milliseconds per (rollout.get's gather, learner.step) at
the reference's shape -- batch 64, net_arch [64, 64] shared, 7 actions, observations of 6 and of 18 values -- and at batch 4096, and, beside it, the same step
done by the torch restatement of tests/ppo_ref.py in float32 on the same GPU, eager (autograd, one launch per operation): that, not this code, is the baseline.

Both sides take their minibatches from `rollout.get(batch_size)` of the same full buffer, so the permutation and the gather are inside both figures; `get`
alone is timed beside them.  Warm-up block first; then blocks of `--epochs` passes over the buffer (more at batch 4096: at least `--min-steps` steps),
alternating between the sides in one process, HIP events around each block, no synchronisation inside a block.
python tools/bench_ppo.py [--blocks 7] [--epochs 2] [--out profiles/r14_ppo.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, '.')
sys.path.insert(0, 'tests')
import torch   # noqa: E402
import ppo_ref as R   # noqa: E402
from human_robot_gym_amd._cstruct import CONST   # noqa: E402
from human_robot_gym_amd.ppo import PpoLearner   # noqa: E402
from human_robot_gym_amd.rollout import RolloutBuffer, build_rollout_desc   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--epochs", type=int, default=2, help="passes over the buffer per block, at least; more where that is fewer than --min-steps minibatches")
ap.add_argument("--min-steps", type=int, default=128, help="minibatch steps per block, at least")
ap.add_argument("--out", default="profiles/r14_ppo.json")
args = ap.parse_args()
A, ARCH, LR, n_envs, n_steps = 7, [64, 64], 7e-5, 256, 64   # the buffer: 16384 rows, 256 minibatches of 64 or 4 of 4096 per pass


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


out = dict(net_arch=ARCH, act_dim=A, n_envs=n_envs, n_steps=n_steps, blocks=args.blocks, device=torch.cuda.get_device_name(0), cases=[])
rng = np.random.RandomState(0)
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()   # noqa: E731
for K, B in ((6, 64), (18, 64), (6, 4096), (18, 4096)):
    N = n_envs * n_steps
    rb = RolloutBuffer(build_rollout_desc(n_envs, n_steps, list(range(K)), act_dim=A, gamma=0.99, gae_lambda=0.9), seed=1)
    epochs = max(args.epochs, -(-args.min_steps * B // N))
    learner = PpoLearner(K, A, net_arch=ARCH, learning_rate=LR, batch_size=B, n_epochs=epochs, log_std_init=-2.7, ortho_init=False, rollout_size=N, seed=0)
    rb.observe(dev(rng.uniform(-1, 1, (n_envs, 64))))
    for _ in range(n_steps):   # the learner's own policy fills the buffer, so that the ratios start at 1 as in a run
        actions, values, log_probs = learner.policy(rb.observation())
        rb.add_step(actions, values, log_probs, None, dev(rng.uniform(-1, 1, (n_envs, 64))), None, dev(rng.normal(size=n_envs)),
                    torch.from_numpy((rng.uniform(size=n_envs) < 0.01).astype(np.uint8)).cuda(), torch.zeros(n_envs, CONST["HRG_INFO_DIM"], dtype=torch.int32).cuda())
    rb.compute_returns_and_advantage(learner.value(rb.observation()))
    ref = R.RefState({k: v.clone() for k, v in learner.state_dict().items()}, torch.float32, device="cuda")
    cfg = R.Cfg(len(ARCH), False, LR, 0.2, None, True, 0.0, 0.5, 0.5)
    steps = epochs * N // B

    def device_block():
        learner.train(rb)

    def eager_block():
        for _ in range(epochs):
            for batch in rb.get(B):
                ref.step(batch, cfg, outputs=False)

    def get_block():
        for _ in range(epochs):
            for batch in rb.get(B):
                pass

    device_block(), eager_block(), get_block()   # warm-up: every kernel and shape of the timed windows
    ms = dict(device=[], eager=[], get=[])
    for _ in range(args.blocks):
        for key, fn in (("device", device_block), ("eager", eager_block), ("get", get_block)):
            ms[key].append(timed(fn) / steps)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = dict(obs_dim=K, batch_size=B, epochs_per_block=epochs, steps_per_block=steps, device_ms_per_step=ms["device"], eager_ms_per_step=ms["eager"], get_ms_per_batch=ms["get"],
               device_ms_median=med["device"], eager_ms_median=med["eager"], get_ms_median=med["get"], device_ms_spread=float(np.max(ms["device"]) - np.min(ms["device"])),
               eager_ms_spread=float(np.max(ms["eager"]) - np.min(ms["eager"])), eager_over_device=med["eager"] / med["device"],
               finite=bool(all(torch.isfinite(v).all() for v in learner.state_dict().values())), n_updates=learner.n_updates)
    print("obs %2d batch %4d: device %.4f ms per minibatch step (gather included; blocks %s), torch eager float32 %.4f ms (blocks %s): %.1f x; get alone %.4f ms"
          % (K, B, med["device"], " ".join("%.4f" % x for x in ms["device"]), med["eager"], " ".join("%.3f" % x for x in ms["eager"]), res["eager_over_device"], med["get"]),
          flush=True)
    out["cases"].append(res)
    learner.close()
    rb.close()
os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
