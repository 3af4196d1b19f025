"""What the device replay buffer costs (csrc/hrgym_replay.h), written to profiles/r11_replay.json (or --out PATH):
  * ms per 4096-env ReachHuman step with and without `add_step` behind it: alternating blocks of 100 steps (train_freq) on ONE batch in one run (HIP events
    around each block), as tools/rollout_time.py; the step kernel is the same code object in both, and finished envs restart alike.  Two layouts: the ICRA one
    (R-SAC.yaml: obs_keys [goal_difference], 6 values, dataset_obs_norm without squash) and, to set beside r10, the PPO layout of 18 plain values;
  * ms per sample(128) and sample(4096) on a full buffer of 1 000 000 transitions (HIP events around 200 calls), and the bytes each call moves against the
    card's HBM figure;
  * the bytes the buffer holds for the ICRA buffer_size at 4096 envs.
python tools/replay_time.py [--out PATH]"""
import json
import os
import sys
import numpy as np
sys.path.insert(0, '.')
import torch
import human_robot_gym_amd as hrg
from human_robot_gym_amd._lib import HipBatch
from human_robot_gym_amd.mixed import task_clips
from human_robot_gym_amd.replay import ReplayBuffer, build_replay_desc

n, block, rounds, buffer_size = 4096, 100, 6, 1_000_000
HBM_PEAK, HBM_MEASURED = 8.0e12, 6.29e12   # bytes/s: spec, and a float4 copy on this card
clips = task_clips("ReachHuman", 13)
kw = dict(shield_type="SSM", horizon=100, seed=1234)
desc = hrg.build_model_desc(kw, n_clips=clips.n_clips)
B = HipBatch(desc, clips, n)
rng = np.random.RandomState(0)
layouts = {"icra": dict(obs_cols=range(12, 18), mean=rng.uniform(-1, 1, 6), std=rng.uniform(0.1, 2, 6)), "ppo18": dict(obs_cols=range(18))}
acts = [torch.from_numpy(rng.uniform(-1, 1, (n, 7))).cuda() for _ in range(8)]
acts32 = [a.float() for a in acts]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


out = dict(n_envs=n, block=block, buffer_size=buffer_size)
for name, lay in layouts.items():
    rb = ReplayBuffer(build_replay_desc(n, buffer_size, act_dim=7, **lay))
    B.reset()
    B.stagger_episode_phases(100)
    rb.observe(B.obs)

    def plain(k):
        B.step(acts[k % 8].clone())

    def with_add(k):
        B.step(acts[k % 8].clone())
        rb.add_step(acts32[k % 8], B.obs, B.term_obs, B.reward, B.done, B.info)

    for k in range(block):   # warm-up: every kernel and shape of the timed windows
        with_add(k)
    ms = {"step": [], "step_add": []}
    for r in range(rounds):
        for key, fn in (("step", plain), ("step_add", with_add)):
            if key == "step_add":
                rb.observe(B.obs)   # the plain block moved the envs on: the transitions start from the rows on the device
            ms[key].append(timed(lambda: [fn(k) for k in range(block)]) / block)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = dict(obs_dim=rb.obs_dim, capacity=rb.capacity, memory_bytes=rb.memory_bytes(), step_ms=ms["step"], step_add_ms=ms["step_add"], step_ms_median=med["step"],
               step_add_ms_median=med["step_add"], add_us_difference_of_medians=1e3 * (med["step_add"] - med["step"]),
               add_share_of_block=(med["step_add"] - med["step"]) / med["step_add"], step_ms_spread=float(np.max(ms["step"]) - np.min(ms["step"])),
               step_add_ms_spread=float(np.max(ms["step_add"]) - np.min(ms["step_add"])))
    for key, v in ms.items():
        print("%-6s %-9s ms per %d-env step, blocks of %d alternating: %s  median %.4f" % (name, key, n, block, " ".join("%.4f" % x for x in v), med[key]))
    print("%-6s add: %.1f us per step as a difference of medians (%.1f %% of the block); block-to-block spread %.1f us (step), %.1f us (step + add); %d bytes held"
          % (name, res["add_us_difference_of_medians"], 100 * res["add_share_of_block"], 1e3 * res["step_ms_spread"], 1e3 * res["step_add_ms_spread"], res["memory_bytes"]))
    if name == "icra":   # the sampler on a full buffer of the ICRA size
        while not rb.full:
            rb.add_step(acts32[0], B.obs, B.term_obs, B.reward, B.done, B.info)
        K, A = rb.obs_dim, rb.act_dim
        for bs in (128, 4096):
            rb.sample(bs)
            per_call = timed(lambda: [rb.sample(bs) for _ in range(200)]) / 200
            moved = bs * (2 * (2 * K + A) * 4 + 4 + 2 + 8)   # read: two observation rows, the action, reward, done, timeout; written: the same rows and two scalars
            res["sample_%d" % bs] = dict(ms_per_call=per_call, bytes_moved=moved, bytes_per_s=moved / (per_call * 1e-3), share_of_hbm_peak=moved / (per_call * 1e-3) / HBM_PEAK,
                                         share_of_hbm_measured=moved / (per_call * 1e-3) / HBM_MEASURED)
            print("sample(%d) on %d transitions: %.4f ms per call (five output allocations and one launch), %d bytes moved: %.3g bytes/s = %.4f %% of the %.1f TB/s peak"
                  % (bs, rb.capacity * n, per_call, moved, res["sample_%d" % bs]["bytes_per_s"], 100 * res["sample_%d" % bs]["share_of_hbm_peak"], HBM_PEAK / 1e12))
    out[name] = res
    rb.close()
B.close()
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "profiles/r11_replay.json"
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
