"""What the device replay buffer costs (csrc/hrgym_her.h), written to profiles/r08_her.json (or --out PATH):
  * ms per 4096-env ReachHuman step with and without the add kernel behind it: alternating blocks of 50 steps on ONE batch in one run (HIP events around each
    block), as tools/dataset_step_time.py; the step kernel is the same code object in both, and finished envs restart alike;
  * ms per sample() call at B = 256, 4096 and 65536 from a full buffer of 4096 x 256 transitions (wall clock over 20 calls each: a call reads the prefix sum's
    total back, so it ends with a stream synchronisation);
  * for the record, the host route this replaces: two observation rows per env, reward, done and info to the host every step, and a numpy gather +
    numpy compute_reward per batch.
python tools/her_time.py [--host] [--out PATH]"""
import json
import os
import sys
import time
import numpy as np
sys.path.insert(0, '.')
import torch
import human_robot_gym_amd as hrg
from human_robot_gym_amd._lib import HipBatch
from human_robot_gym_amd.her import HerBuffer, build_her_desc
from human_robot_gym_amd.mixed import task_clips

n, cap, block, rounds = 4096, 256, 50, 6
clips = task_clips("ReachHuman", 13)
kw = dict(shield_type="SSM", horizon=100, seed=1234, reward_shaping=False)
desc = hrg.build_model_desc(kw, n_clips=clips.n_clips)
B = HipBatch(desc, clips, n)
cols = list(range(0, 12)) + list(range(18, 33)) + list(range(33, 39))   # the goal-env wrapper's default view
her = HerBuffer(build_her_desc(n, cap, 100, "reach", cols, model_desc=desc, seed=1))
B.reset()
B.stagger_episode_phases(100)
her.observe(B.obs)
rng = np.random.RandomState(0)
acts = [torch.from_numpy(rng.uniform(-1, 1, (n, 7))).cuda() for _ in range(8)]


def plain(a):
    B.step(a)


def with_add(a):
    B.step(a)
    her.add_step(a, B.obs, B.term_obs, B.reward, B.done, B.info)


for k in range(100):
    with_add(acts[k % 8].clone())
ms = {"step": [], "step_add": []}
for r in range(rounds):
    for name, fn in (("step", plain), ("step_add", with_add)):
        rows = [acts[k % 8].clone() for k in range(block)]
        if name == "step_add":
            her.observe(B.obs)   # the plain block moved the envs on: the buffer's open episodes start again from the rows on the device
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for a in rows:
            fn(a)
        e1.record()
        torch.cuda.synchronize()
        ms[name].append(e0.elapsed_time(e1) / block)
out = dict(n_envs=n, capacity=cap, block=block, step_ms=ms["step"], step_add_ms=ms["step_add"], step_ms_median=float(np.median(ms["step"])),
           step_add_ms_median=float(np.median(ms["step_add"])), add_us_difference_of_medians=1e3 * float(np.median(ms["step_add"]) - np.median(ms["step"])),
           step_ms_spread=float(np.max(ms["step"]) - np.min(ms["step"])), step_add_ms_spread=float(np.max(ms["step_add"]) - np.min(ms["step_add"])))
for name, v in ms.items():
    print("%-9s ms per %d-env step, blocks of %d alternating: %s  median %.4f" % (name, n, block, " ".join("%.4f" % x for x in v), float(np.median(v))))
print("add kernel: %.1f us per step as a difference of medians; block-to-block spread %.1f us (step), %.1f us (step + add)"
      % (out["add_us_difference_of_medians"], 1e3 * out["step_ms_spread"], 1e3 * out["step_add_ms_spread"]))
for k in range(cap):   # until every ring has wrapped
    with_add(acts[k % 8].clone())
stored, closed, _ = her.counts_host()
out.update(stored=stored, closed=closed, sample_ms={})
print("buffer: %d transitions stored, %d of finished episodes" % (stored, closed))
for bs in (256, 4096, 65536):
    her.sample(bs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        her.sample(bs)
    torch.cuda.synchronize()
    out["sample_ms"][str(bs)] = 1e3 * (time.perf_counter() - t0) / 20
    print("sample(%d): %.3f ms per call" % (bs, out["sample_ms"][str(bs)]))
if "--host" in sys.argv:   # the route this replaces
    steps = 20
    hp, hq = np.zeros((n, cap, 64), np.float32), np.zeros((n, cap, 64), np.float32)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        obs, rew, done, info = B.step(acts[k % 8].clone())
        s = k % cap
        hq[:, s] = np.where(done.cpu().numpy()[:, None] != 0, B.term_obs.cpu().numpy(), obs.cpu().numpy())
        hp[:, s] = obs.cpu().numpy()
        rew.cpu().numpy(), info.cpu().numpy()
    out["host_step_ms"] = 1e3 * (time.perf_counter() - t0) / steps
    print("host route, step + rows / reward / done / info to the host: %.2f ms per step over %d steps" % (out["host_step_ms"], steps))
    out["host_sample_ms"] = {}
    for bs in (256, 4096, 65536):
        t0 = time.perf_counter()
        for _ in range(5):
            e, s, g = rng.randint(0, n, bs), rng.randint(0, cap, bs), rng.randint(0, cap, bs)
            pre, post, goal = hp[e, s], hq[e, s], hq[e, g][:, 18:24]
            dist = np.linalg.norm(post[:, 18:24].astype(np.float64) - goal, axis=-1)
            r = np.where(dist <= desc.goal_dist, desc.task_reward, -1.0) * desc.reward_scale
            batch = [torch.from_numpy(x).cuda() for x in (pre[:, cols], post[:, cols], goal, r)]
        torch.cuda.synchronize()
        out["host_sample_ms"][str(bs)] = 1e3 * (time.perf_counter() - t0) / 5
        print("host route, numpy gather + reward + upload of %d samples: %.3f ms per call" % (bs, out["host_sample_ms"][str(bs)]))
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "profiles/r08_her.json"
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
her.close()
B.close()
