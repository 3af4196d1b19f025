"""What an evaluation step costs (csrc/hrgym_eval.h), written to profiles/r15_eval.json (or --out PATH): ms per step of 4096 ReachHuman envs (SSM shield,
horizon 100) under a deterministic SAC actor of net_arch [64, 64, 64],
  * in the device loop of HipVecEnv.evaluate: the fused actor, the step, the ledger -- three launches, HIP events around blocks of 100 steps;
  * in the host loop, the only way to run the same policy without the loop: learner.act(deterministic=True) on the uploaded observation, torch's unscaling,
    env.step through the host with its info dicts (what evaluate_policy reads the episodes from) -- a host clock around blocks of 100 steps, each ending in
    the step's own synchronising copy;
  * each of the three launches alone, back to back in blocks of 100 (HIP events): the per-launch split;
  * one whole env.evaluate(learner, 4096) with sync_every 16, by the host clock: the loop with its readbacks and the export.
The two loops alternate, block by block, on two envs of one seed in one run.
python tools/eval_time.py [--out PATH] [--n-envs N]"""
import json
import os
import sys
import time

import numpy as np
sys.path.insert(0, '.')
import torch   # noqa: E402
import human_robot_gym_amd as hrg   # noqa: E402
from human_robot_gym_amd.evaluation import Evaluator   # noqa: E402
from human_robot_gym_amd.sac import SacLearner   # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


n, block, rounds = arg("--n-envs", 4096), 100, 4
kw = dict(env_kwargs=dict(shield_type="SSM", horizon=100, seed=1234))
dev_env, host_env = hrg.HipVecEnv(n, **kw), hrg.HipVecEnv(n, **kw)
K, A = dev_env.observation_space.shape[0], dev_env.action_space.shape[0]
learner = SacLearner(K, A, net_arch=[64, 64, 64], batch_size=128, seed=0)
low, high = (torch.from_numpy(np.asarray(x, np.float64)).cuda() for x in (host_env.action_space.low, host_env.action_space.high))


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


# the device loop, as HipVecEnv.evaluate runs it (without the readbacks: they are one per sync_every steps)
be = dev_env._backend
b = be.batch
be.reset_device()
b.stagger_episode_phases(100)
# 16 episodes per env: a quota no env meets inside the timed windows (9 episodes), so every done step writes its record
ev = Evaluator(dev_env._eval_desc(n, 1, 16 * n), device=0, info_keys=dev_env._info_keys)
ev.begin(b.obs)


def device_step():
    be.launch_step(ev.policy(learner))
    ev.step(b.obs, b.reward, b.done, b.info)


state = dict(obs=host_env.reset())


def host_step():
    a = learner.act(torch.from_numpy(np.ascontiguousarray(state["obs"])).cuda(), deterministic=True)
    state["obs"], _, _, _ = host_env.step((low + 0.5 * (a.to(torch.float64) + 1.0) * (high - low)).cpu().numpy())


for _ in range(block):   # warm-up: every kernel and shape of the timed windows
    device_step()
    host_step()
ms = {"device_loop": [], "host_loop": []}
for r in range(rounds):
    ms["device_loop"].append(events(lambda: [device_step() for _ in range(block)]) / block)
    ms["host_loop"].append(clock(lambda: [host_step() for _ in range(block)]) / block)
acts = ev.actions.clone()
split = dict(actor=[], step=[], ledger=[])
for r in range(rounds):
    split["actor"].append(events(lambda: [ev.policy(learner) for _ in range(block)]) / block)
    split["step"].append(events(lambda: [be.launch_step(acts.clone()) for _ in range(block)]) / block)   # (with the clone of the action rows the step may rewrite)
    split["ledger"].append(events(lambda: [ev.step(b.obs, b.reward, b.done, b.info) for _ in range(block)]) / block)
ev.close()
whole_ms = clock(lambda: state.update(result=dev_env.evaluate(learner, n, sync_every=16)))
res = state["result"]
steps_run = -(-(int(res.step.max()) + 1) // 16) * 16
med = {k: float(np.median(v)) for k, v in {**ms, **split}.items()}
out = dict(n_envs=n, block=block, net_arch=[64, 64, 64], obs_dim=K, act_dim=A, ms_per_step=ms, per_launch_ms=split, median_ms=med,
           host_over_device=med["host_loop"] / med["device_loop"], launches_sum_ms=med["actor"] + med["step"] + med["ledger"],
           spread_ms={k: float(np.max(v) - np.min(v)) for k, v in ms.items()},
           evaluate=dict(n_eval_episodes=n, sync_every=16, steps_run=steps_run, wall_ms=whole_ms, wall_ms_per_step=whole_ms / steps_run, episodes=len(res.episode_rewards),
                         mean_reward=res.mean_reward, std_reward=res.std_reward))
for k, v in {**ms, **split}.items():
    print("%-12s ms per %d-env step, blocks of %d: %s  median %.4f" % (k, n, block, " ".join("%.4f" % x for x in v), med[k]))
print("host loop / device loop: %.1f x; the three launches alone add up to %.4f ms; env.evaluate(%d episodes): %.1f ms for %d steps (%.4f ms per step with readbacks and export)"
      % (out["host_over_device"], out["launches_sum_ms"], n, whole_ms, steps_run, whole_ms / steps_run))
dev_env.close()
host_env.close()
out_path = arg("--out", "profiles/r15_eval.json")
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
