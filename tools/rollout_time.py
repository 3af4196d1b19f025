"""What the device rollout buffer costs (csrc/hrgym_rollout.h), written to profiles/r10_rollout.json (or --out PATH):
  * ms per 4096-env ReachHuman step with and without `view(term_obs)` + `add_step` behind it: alternating blocks of 64 steps (one rollout) on ONE batch in one
    run (HIP events around each block), as tools/her_time.py; the step kernel is the same code object in both, and finished envs restart alike;
  * ms per compute_returns_and_advantage at T = 64 (HIP events around 20 calls);
  * ms per epoch of get() at B = 4096: one randperm and 64 gathers over the 262144 samples (HIP events around each of 5 epochs);
  * with --host, for the record, the host route an on-policy learner takes without the buffer (unchanged by it): HipVecEnv.step for 64 steps, the packed block
    to pinned memory and the numpy views and info dicts every step (wall clock; every step ends in a blocking copy).
python tools/rollout_time.py [--host] [--out PATH]"""
import json
import os
import sys
import time
import numpy as np
sys.path.insert(0, '.')
import torch
import human_robot_gym_amd as hrg
from human_robot_gym_amd._lib import HipBatch
from human_robot_gym_amd.mixed import task_clips
from human_robot_gym_amd.rollout import RolloutBuffer, build_rollout_desc

n, T, rounds, batch_size = 4096, 64, 6, 4096
clips = task_clips("ReachHuman", 13)
kw = dict(shield_type="SSM", horizon=100, seed=1234)   # training/config/human_reach_ppo_parallel.yaml: wrappers safe
desc = hrg.build_model_desc(kw, n_clips=clips.n_clips)
B = HipBatch(desc, clips, n)
rb = RolloutBuffer(build_rollout_desc(n, T, range(18), act_dim=7, gamma=0.99, gae_lambda=0.9))   # algorithm/ppo.yaml
B.reset()
B.stagger_episode_phases(100)
rb.observe(B.obs)
rng = np.random.RandomState(0)
acts = [torch.from_numpy(rng.uniform(-1, 1, (n, 7))).cuda() for _ in range(8)]
acts32 = [a.float() for a in acts]
vals = torch.from_numpy(rng.uniform(-1, 1, n).astype(np.float32)).cuda()


def plain(k):
    B.step(acts[k % 8].clone())


def with_add(k):
    B.step(acts[k % 8].clone())
    term = rb.view(B.term_obs)   # what the value function would be evaluated on
    rb.add_step(acts32[k % 8], vals, vals, term[:, 0].contiguous(), B.obs, B.term_obs, B.reward, B.done, B.info)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


for k in range(T):   # warm-up: every kernel and shape of the timed windows
    with_add(k)
rb.compute_returns_and_advantage(vals)
for _ in rb.get(batch_size):
    pass
ms = {"step": [], "step_view_add": []}
for r in range(rounds):
    for name, fn in (("step", plain), ("step_view_add", with_add)):
        if name == "step_view_add":
            rb.reset()
            rb.observe(B.obs)   # the plain block moved the envs on: the rollout starts from the rows on the device
        ms[name].append(timed(lambda: [fn(k) for k in range(T)]) / T)
out = dict(n_envs=n, n_steps=T, block=T, step_ms=ms["step"], step_view_add_ms=ms["step_view_add"], step_ms_median=float(np.median(ms["step"])),
           step_view_add_ms_median=float(np.median(ms["step_view_add"])),
           view_add_us_difference_of_medians=1e3 * float(np.median(ms["step_view_add"]) - np.median(ms["step"])),
           step_ms_spread=float(np.max(ms["step"]) - np.min(ms["step"])), step_view_add_ms_spread=float(np.max(ms["step_view_add"]) - np.min(ms["step_view_add"])))
for name, v in ms.items():
    print("%-13s ms per %d-env step, blocks of %d alternating: %s  median %.4f" % (name, n, T, " ".join("%.4f" % x for x in v), float(np.median(v))))
print("view + add: %.1f us per step as a difference of medians; block-to-block spread %.1f us (step), %.1f us (step + view + add)"
      % (out["view_add_us_difference_of_medians"], 1e3 * out["step_ms_spread"], 1e3 * out["step_view_add_ms_spread"]))
out["compute_ms"] = timed(lambda: [rb.compute_returns_and_advantage(vals) for _ in range(20)]) / 20
print("compute_returns_and_advantage, T = %d, n = %d: %.4f ms per call" % (T, n, out["compute_ms"]))
out["get_epoch_ms"] = [timed(lambda: [None for _ in rb.get(batch_size)]) for _ in range(5)]
out["get_epoch_ms_median"] = float(np.median(out["get_epoch_ms"]))
print("get(), one epoch of %d batches of %d: %s ms  median %.3f" % (n * T // batch_size, batch_size, " ".join("%.3f" % x for x in out["get_epoch_ms"]), out["get_epoch_ms_median"]))
out["device_rollout_ms"] = T * out["step_view_add_ms_median"] + out["compute_ms"]
print("device route, %d steps with view + add, then compute (no policy): %.2f ms" % (T, out["device_rollout_ms"]))
rb.close()
B.close()
if "--host" in sys.argv:   # the route without the buffer
    env = hrg.HipVecEnv(n, env_kwargs=kw, clips=clips)
    env.reset()
    host_acts = [rng.uniform(-1, 1, (n, 7)) for _ in range(8)]
    for k in range(8):
        env.step(host_acts[k % 8])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(T):
        env.step(host_acts[k % 8])
    out["host_rollout_ms"] = 1e3 * (time.perf_counter() - t0)
    out["host_step_ms"] = out["host_rollout_ms"] / T
    print("host route, HipVecEnv.step x %d (block to pinned memory, numpy views, info dicts; no policy, no buffer): %.2f ms, %.3f ms per step"
          % (T, out["host_rollout_ms"], out["host_step_ms"]))
    env.close()
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "profiles/r10_rollout.json"
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
