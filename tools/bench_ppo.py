"""What one PPO minibatch step costs on the device (csrc/hrgym_ppo.h), written to profiles/r14_ppo.json: milliseconds per (rollout.get's gather, learner.step) at
the reference's shape -- batch 64, net_arch [64, 64] shared, 7 actions, observations of 6 and of 18 values -- and at batch 4096, and, beside it, the same step
done by the torch restatement of tests/ppo_ref.py in float32 on the same GPU, eager (autograd, one launch per operation): that, not this code, is the baseline.

Both sides take their minibatches from `rollout.get(batch_size)` of the same full buffer, so the permutation and the gather are inside both figures; `get`
alone is timed beside them.  Warm-up block first; then blocks of `--epochs` passes over the buffer (more at batch 4096: at least `--min-steps` steps),
alternating between the sides in one process, HIP events around each block, no synchronisation inside a block.
python tools/bench_ppo.py [--blocks 7] [--epochs 2] [--out profiles/r14_ppo.json]

--population P [P ...]: instead, what one minibatch step of a population of P members costs at the reference's shape -- observations of 18 values,
7 actions, net_arch [64, 64] shared, batch 64 per member -- on fixed minibatches, the steps alone; 0 stands for the lone PpoLearner through its own class.  Blocks of
--min-steps steps, the sizes taking turns within a round, HIP events around each block.  With --train also one train() of the reference's rollout (10 envs per
member, n_steps 64, 20 epochs: 200 minibatch steps with their permutations and gathers) for the largest P, beside that many lone train() calls in turn.
python tools/bench_ppo.py --population 0 1 2 5 16 --train --out profiles/r23_ppo_population.json

--distinct (with --population): every member gets its own learning rate, clip ranges, ent_coef, vf_coef and max_grad_norm, so that the step reads a table the
caller uploaded instead of the one the scalar arguments fill."""
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
ap.add_argument("--population", type=int, nargs="+", default=None, help="time the step of populations of these sizes instead (0: the lone learner)")
ap.add_argument("--distinct", action="store_true", help="with --population: distinct hyper-parameters per member")
ap.add_argument("--train", action="store_true", help="with --population: also one train() of the reference's rollout shape against lone train() calls in turn")
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


rng = np.random.RandomState(0)
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()   # noqa: E731


def filled_buffer(n, K, policy, value, seed=1):
    """A full, computed buffer of `n` envs that `policy` filled, so that the ratios start at 1 as in a run."""
    rb = RolloutBuffer(build_rollout_desc(n, n_steps, list(range(K)), act_dim=A, gamma=0.99, gae_lambda=0.9), seed=seed)
    rb.observe(dev(rng.uniform(-1, 1, (n, 64))))
    for _ in range(n_steps):
        actions, values, log_probs = policy(rb.observation())
        rb.add_step(actions, values, log_probs, None, dev(rng.uniform(-1, 1, (n, 64))), None, dev(rng.normal(size=n)),
                    torch.from_numpy((rng.uniform(size=n) < 0.01).astype(np.uint8)).cuda(), torch.zeros(n, CONST["HRG_INFO_DIM"], dtype=torch.int32).cuda())
    rb.compute_returns_and_advantage(value(rb.observation()))
    return rb


def population_bench():
    from human_robot_gym_amd.rollout import RolloutBufferSamples
    K, B, kw = 18, 64, dict(net_arch=ARCH, learning_rate=LR, batch_size=64, n_epochs=20, log_std_init=-2.7, ortho_init=False)
    res = dict(obs_dim=K, act_dim=A, net_arch=ARCH, batch_size=B, blocks=args.blocks, steps_per_block=args.min_steps, device=torch.cuda.get_device_name(0), step=[])
    sides = []
    for P in args.population:
        if P:
            from human_robot_gym_amd.ppo import PpoPopulation
            hyper = {}
            if args.distinct:
                hyper = dict(learning_rate=[LR * (1.0 + 0.1 * p) for p in range(P)], clip_range=[0.2 + 0.01 * p for p in range(P)],
                             clip_range_vf=[None if p % 2 == 0 else 0.2 + 0.01 * p for p in range(P)], ent_coef=[0.001 * p for p in range(P)],
                             vf_coef=[0.5 + 0.01 * p for p in range(P)], max_grad_norm=[0.5 + 0.05 * p for p in range(P)])
            learner = PpoPopulation(K, A, P, list(range(P)), **{**kw, **hyper})
        else:
            learner = PpoLearner(K, A, seed=0, **kw)
        obs = dev(rng.uniform(-1, 1, (max(P, 1) * B, K)))
        actions, values, log_probs = learner.policy(obs)
        batch = RolloutBufferSamples(obs, actions, values, log_probs, dev(rng.normal(size=max(P, 1) * B)), dev(rng.normal(size=max(P, 1) * B)))
        sides.append((P, learner, batch, []))
    for _, learner, batch, _ in sides:   # warm-up
        for _ in range(args.min_steps):
            learner.step(batch)
    for _ in range(args.blocks):
        for _, learner, batch, ms in sides:
            ms.append(timed(lambda: [learner.step(batch) for _ in range(args.min_steps)]) / args.min_steps)
    for P, learner, _, ms in sides:
        res["step"].append(dict(population=P, distinct=bool(args.distinct and P), ms_per_step=ms, ms_median=float(np.median(ms)), ms_spread=float(np.max(ms) - np.min(ms)),
                                finite=bool(torch.isfinite(learner.p.params).all()), n_updates=learner.n_updates))
        print("population %2d: %.4f ms per minibatch step (blocks %s)" % (P, np.median(ms), " ".join("%.4f" % x for x in ms)), flush=True)
        learner.close()
    P = max(args.population)
    if args.train and P:
        from human_robot_gym_amd.ppo import PpoPopulation
        m = 10
        pop = PpoPopulation(K, A, P, list(range(P)), rollout_size=m * n_steps, **kw)
        big = filled_buffer(P * m, K, pop.policy, pop.value)
        lones = [PpoLearner(K, A, seed=p, rollout_size=m * n_steps, **kw) for p in range(P)]
        bufs = [filled_buffer(m, K, lone.policy, lone.value, seed=p) for p, lone in enumerate(lones)]
        together = lambda: pop.train(big)                                             # noqa: E731
        in_turn = lambda: [lone.train(rb) for lone, rb in zip(lones, bufs)]           # noqa: E731
        together(), in_turn()
        ms = dict(population=[], lone_in_turn=[])
        for _ in range(args.blocks):
            ms["population"].append(timed(together))
            ms["lone_in_turn"].append(timed(in_turn))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        res["train"] = dict(population=P, envs_per_member=m, n_steps=n_steps, n_epochs=20, minibatch_steps=20 * m * n_steps // B, population_ms=ms["population"],
                            lone_in_turn_ms=ms["lone_in_turn"], population_ms_median=med["population"], lone_in_turn_ms_median=med["lone_in_turn"],
                            lone_over_population=med["lone_in_turn"] / med["population"])
        print("train(): population of %d %.2f ms, %d lone learners in turn %.2f ms: %.2f x" % (P, med["population"], P, med["lone_in_turn"], res["train"]["lone_over_population"]), flush=True)
        for h in [pop, big] + lones + bufs:
            h.close()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if args.population is not None:
    population_bench()
    sys.exit(0)
out = dict(net_arch=ARCH, act_dim=A, n_envs=n_envs, n_steps=n_steps, blocks=args.blocks, device=torch.cuda.get_device_name(0), cases=[])
for K, B in ((6, 64), (18, 64), (6, 4096), (18, 4096)):
    N = n_envs * n_steps
    epochs = max(args.epochs, -(-args.min_steps * B // N))
    learner = PpoLearner(K, A, net_arch=ARCH, learning_rate=LR, batch_size=B, n_epochs=epochs, log_std_init=-2.7, ortho_init=False, rollout_size=N, seed=0)
    rb = filled_buffer(n_envs, K, learner.policy, learner.value)   # the learner's own policy fills the buffer
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
