"""ms per 4096-env step through hrg_batch_step_imitation (expert + reward kernels around the step kernel) against hrg_batch_step: alternating blocks of
both entry points on ONE batch of this build in one run (HIP events around each block of 50 steps); the step kernel is the same code through both.  During
the plain blocks the expert's noise and episode sums stand still; they carry no weight in the timing (every env runs the same instructions either way).
python tools/imitation_step_time.py [--env ReachHuman|PickPlaceHumanCart]   (the two tasks whose expert has the task's name and no required argument)"""
import sys
import numpy as np
sys.path.insert(0, '.')
import torch
import human_robot_gym_amd as hrg
from human_robot_gym_amd._lib import HipBatch
from human_robot_gym_amd.expert import build_expert_desc
from human_robot_gym_amd.mixed import task_clips, task_env_kwargs

env_id = sys.argv[sys.argv.index("--env") + 1] if "--env" in sys.argv else "ReachHuman"
if env_id not in ("ReachHuman", "PickPlaceHumanCart"):
    sys.exit("--env: ReachHuman or PickPlaceHumanCart")
cart = env_id != "ReachHuman"
n, block, rounds = 4096, 50, 6
clips = task_clips(env_id, 13)
kw = dict(shield_type="SSM", horizon=100, seed=1234, reward_shaping=True, **task_env_kwargs(env_id))
B = HipBatch(hrg.build_model_desc(kw, n_clips=clips.n_clips, env_id=env_id, ik_position_delta=dict(action_limit=0.1) if cart else None), clips, n)
lo, hi = ([-0.1] * 3 + [-1.0], [0.1] * 3 + [1.0]) if cart else ([-1.0] * 7, [1.0] * 7)
B.attach_expert(build_expert_desc(dict(id=env_id, signal_to_noise_ratio=0.98, seed=1), lo, hi, dict(alpha=0.25, beta=0.7, iota_m=0.1, iota_g=0.5)))
B.reset()
B.stagger_episode_phases(100)
rng = np.random.RandomState(0)
acts = []
for _ in range(8):
    a = np.zeros((n, 7)); a[:, :len(lo)] = rng.uniform(lo, hi, (n, len(lo)))
    acts.append(torch.from_numpy(a).cuda())
for k in range(100):
    B.step(acts[k % 8].clone())
ms = {"step": [], "step_imitation": []}
for r in range(rounds):
    for name in ("step", "step_imitation"):
        fn = getattr(B, name)
        rows = [acts[k % 8].clone() for k in range(block)]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for a in rows:
            fn(a)
        e1.record()
        torch.cuda.synchronize()
        ms[name].append(e0.elapsed_time(e1) / block)
for name, v in ms.items():
    print("%s %-15s ms per %d-env step, blocks of %d alternating: %s  median %.4f" % (env_id, name, n, block, " ".join("%.4f" % x for x in v), float(np.median(v))))
print("difference of the medians: %.1f us per step (two extra launches)" % (1e3 * (np.median(ms["step_imitation"]) - np.median(ms["step"]))))
B.close()
