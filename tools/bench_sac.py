"""What one SAC gradient step costs on the device (csrc/hrgym_sac.h), written to profiles/r12_sac.json: milliseconds per (replay.sample, learner.step) at the ICRA
shape -- batch 128, net_arch [64, 64, 64], 4 actions, observations of 6 and of 18 values -- and, beside it, the same step done by the torch restatement of
tests/sac_ref.py in float32 on the same GPU, eager (autograd, one launch per operation): that, not this code, is the baseline.

Both sides draw their batches with replay.sample from the same full buffer; the baseline draws its noise with torch.randn.  Warm-up block first; then blocks of
`--steps` gradient steps, alternating between the two sides in one process, HIP events around each block, no synchronisation inside a block.
python tools/bench_sac.py [--blocks 7] [--steps 200]

--population P [P ...] times the step of a population instead (sac.SacPopulation: P learners in the same six launches), written to
profiles/r21_sac_population.json: milliseconds per (replay.sample_groups, population.step) over P groups of 64 envs at the same shapes, and that time per member.
No eager baseline: the figure to compare with is P lone steps.
python tools/bench_sac.py --population 1 2 4 5 8 16 32 64

--distinct (with --population): every member gets its own learning rate, gamma, tau, target entropy and entropy coefficient (every third one fixed), so that the
step reads a table the caller uploaded instead of the one the scalar arguments fill."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, '.')
sys.path.insert(0, 'tests')
import torch   # noqa: E402
import sac_ref as R   # noqa: E402
from human_robot_gym_amd._cstruct import CONST   # noqa: E402
from human_robot_gym_amd.replay import ReplayBuffer, build_replay_desc   # noqa: E402
from human_robot_gym_amd.sac import SacLearner, SacPopulation   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--population", type=int, nargs="+", default=None, help="time a population of this many members (several: one after the other)")
ap.add_argument("--distinct", action="store_true", help="with --population: distinct hyper-parameters per member")
ap.add_argument("--out", default=None, help="default: profiles/r12_sac.json, with --population profiles/r21_sac_population.json")
args = ap.parse_args()
if args.out is None:
    args.out = "profiles/r21_sac_population.json" if args.population else "profiles/r12_sac.json"
B, A, ARCH, LR, n_envs, slots = 128, 4, [64, 64, 64], 5e-4, 64, 16


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def full_buffer(rng, n_envs, K):
    """A replay buffer of `n_envs` envs with every slot filled."""
    rb = ReplayBuffer(build_replay_desc(n_envs, n_envs * slots, list(range(K)), act_dim=A, seed=1))
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()   # noqa: E731
    rb.observe(dev(rng.uniform(-1, 1, (n_envs, 64))))
    for _ in range(slots):
        rb.add_step(dev(rng.uniform(-1, 1, (n_envs, A))), dev(rng.uniform(-1, 1, (n_envs, 64))), dev(rng.uniform(-1, 1, (n_envs, 64))), dev(rng.normal(size=n_envs)),
                    torch.from_numpy((rng.uniform(size=n_envs) < 0.05).astype(np.uint8)).cuda(), torch.zeros(n_envs, CONST["HRG_INFO_DIM"], dtype=torch.int32).cuda())
    return rb


out = dict(batch_size=B, net_arch=ARCH, act_dim=A, steps_per_block=args.steps, blocks=args.blocks, device=torch.cuda.get_device_name(0))
rng = np.random.RandomState(0)
for P in args.population or ():
    for K in (6, 18):
        rb = full_buffer(rng, P * n_envs, K)
        hyper = dict(learning_rate=LR, ent_coef="auto_0.2")
        if args.distinct:
            hyper = dict(learning_rate=[LR * (1.0 + 0.1 * p) for p in range(P)], gamma=[0.99 - 0.001 * p for p in range(P)], tau=[0.005 + 0.001 * p for p in range(P)],
                         ent_coef=[0.1 + 0.01 * p if p % 3 == 2 else "auto_%g" % (0.2 + 0.01 * p) for p in range(P)], target_entropy=[-float(A) - 0.1 * p for p in range(P)])
        pop = SacPopulation(K, A, P, list(range(P)), net_arch=ARCH, batch_size=B, **hyper)
        pop.train(rb, args.steps)   # warm-up
        ms = [timed(lambda: pop.train(rb, args.steps)) / args.steps for _ in range(args.blocks)]
        med = float(np.median(ms))
        out["population_%d_obs_%d" % (P, K)] = dict(n_members=P, obs_dim=K, distinct=bool(args.distinct), ms_per_step=ms, ms_median=med, ms_spread=float(np.max(ms) - np.min(ms)), ms_per_member=med / P,
                                                   finite=bool(torch.isfinite(pop.p.params).all()), n_updates=pop.n_updates)
        print("population %2d, obs %2d: %.4f ms per population step (sampling included; blocks %s), %.4f ms per member" % (P, K, med, " ".join("%.4f" % x for x in ms), med / P))
        pop.close()
        rb.close()
for K in () if args.population else (6, 18):
    rb = full_buffer(rng, n_envs, K)
    learner = SacLearner(K, A, net_arch=ARCH, learning_rate=LR, ent_coef="auto_0.2", batch_size=B, seed=0)
    ref = R.RefState({k: v.clone() for k, v in learner.state_dict().items()}, torch.float32, device="cuda")
    cfg = R.Cfg(len(ARCH), LR, 0.99, 0.005, True, 0.2, -float(A), 1)

    def device_block():
        learner.train(rb, args.steps)

    def eager_block():
        for _ in range(args.steps):
            ref.step(rb.sample(B), torch.randn(B, A, device="cuda"), torch.randn(B, A, device="cuda"), cfg, outputs=False)

    def sample_block():
        for _ in range(args.steps):
            rb.sample(B)

    device_block(), eager_block(), sample_block()   # warm-up: every kernel and shape of the timed windows
    ms = dict(device=[], eager=[], sample=[])
    for _ in range(args.blocks):
        for key, fn in (("device", device_block), ("eager", eager_block), ("sample", sample_block)):
            ms[key].append(timed(fn) / args.steps)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = dict(obs_dim=K, device_ms_per_step=ms["device"], eager_ms_per_step=ms["eager"], sample_ms_per_call=ms["sample"], device_ms_median=med["device"],
               eager_ms_median=med["eager"], sample_ms_median=med["sample"], device_ms_spread=float(np.max(ms["device"]) - np.min(ms["device"])),
               eager_ms_spread=float(np.max(ms["eager"]) - np.min(ms["eager"])), eager_over_device=med["eager"] / med["device"],
               finite=bool(all(torch.isfinite(v).all() for v in learner.state_dict().values())), n_updates=learner.n_updates)
    print("obs %2d: device %.4f ms per gradient step (sampling included; blocks %s), torch eager float32 %.4f ms (blocks %s): %.1f x; sample alone %.4f ms"
          % (K, med["device"], " ".join("%.4f" % x for x in ms["device"]), med["eager"], " ".join("%.3f" % x for x in ms["eager"]), res["eager_over_device"], med["sample"]))
    out["obs_%d" % K] = res
    learner.close()
    rb.close()
os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
