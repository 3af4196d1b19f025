"""ms per 4096-env step through hrg_batch_step_dataset (state reward + restore kernels behind the step kernel) against hrg_batch_step: alternating blocks of
both entry points on ONE batch of this build in one run (HIP events around each block of 50 steps), as tools/imitation_step_time.py; the step kernel is the
same code through both.  The dataset is collected first, at 64 envs.  During the plain blocks finished envs start fresh episodes, during the dataset blocks
from dataset states.  Also, once, the per-env host route for the record: set_states of every finished env + the reward rule in numpy.
python tools/dataset_step_time.py [--env ReachHuman|PickPlaceHumanCart] [--rsi 0|1] [--host]"""
import sys
import time
import numpy as np
sys.path.insert(0, '.')
sys.path.insert(0, 'tests')
import torch
import human_robot_gym_amd as hrg
from human_robot_gym_amd._lib import HipBatch
from human_robot_gym_amd.dataset import collect_expert_dataset
from human_robot_gym_amd.mixed import task_clips, task_env_kwargs

env_id = sys.argv[sys.argv.index("--env") + 1] if "--env" in sys.argv else "ReachHuman"
rsi = float(sys.argv[sys.argv.index("--rsi") + 1]) if "--rsi" in sys.argv else 0.0
if env_id not in ("ReachHuman", "PickPlaceHumanCart"):
    sys.exit("--env: ReachHuman or PickPlaceHumanCart")
cart = env_id != "ReachHuman"
n, block, rounds = 4096, 50, 6
clips = task_clips(env_id, 13)
kw = dict(shield_type="SSM", horizon=100, seed=1234, reward_shaping=True, **task_env_kwargs(env_id))
ik = dict(action_limit=0.1) if cart else None
ds = collect_expert_dataset(env_id, 64, 64, expert=dict(id=env_id, signal_to_noise_ratio=0.98, seed=1), env_kwargs=kw, clips=clips, ik_position_delta=ik)
print("%s dataset: %d episodes, %d transitions, %.1f MB on the device" % (env_id, ds.n_episodes, ds.total_T, (ds.states.nbytes + (0 if ds.boxes is None else ds.boxes.nbytes) + ds.obs.nbytes) / 1e6))
B = HipBatch(hrg.build_model_desc(kw, n_clips=clips.n_clips, env_id=env_id, ik_position_delta=ik), clips, n)
sir = dict(alpha=0.25, iota=0.1) if not cart else dict(alpha=0.25, beta=0.7, iota_m=0.1, iota_g=0.05)
B.attach_dataset(ds, rsi_prob=rsi, state_imitation_reward=sir, seed=1)
B.dataset_reset()
B.stagger_episode_phases(100)
lo, hi = ([-0.1] * 3 + [-1.0], [0.1] * 3 + [1.0]) if cart else ([-1.0] * 7, [1.0] * 7)
rng = np.random.RandomState(0)
acts = []
for _ in range(8):
    a = np.zeros((n, 7)); a[:, :len(lo)] = rng.uniform(lo, hi, (n, len(lo)))
    acts.append(torch.from_numpy(a).cuda())
for k in range(100):
    B.step_dataset(acts[k % 8].clone())
ms = {"step": [], "step_dataset": []}
fin = []
for r in range(rounds):
    for name in ("step", "step_dataset"):
        fn = getattr(B, name)
        rows = [acts[k % 8].clone() for k in range(block)]
        nd = torch.zeros((), dtype=torch.int64, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for a in rows:
            fn(a)
        e1.record()
        torch.cuda.synchronize()
        ms[name].append(e0.elapsed_time(e1) / block)
for name, v in ms.items():
    print("%s rsi_prob %g %-13s ms per %d-env step, blocks of %d alternating: %s  median %.4f" % (env_id, rsi, name, n, block, " ".join("%.4f" % x for x in v), float(np.median(v))))
print("difference of the medians: %.1f us per step (two extra launches + the copies of the finished envs, ~%.0f per step at horizon 100)"
      % (1e3 * (np.median(ms["step_dataset"]) - np.median(ms["step"])), n / 100))
if "--host" in sys.argv:   # the route this replaces: the done mask to the host, set_states of the finished envs, the reward rule in numpy
    import sir_ref as R
    from human_robot_gym_amd._cstruct import BoxState, EnvState
    kind = "pick_place" if cart else "reach"
    states = ds.restore_states()
    t0 = time.perf_counter()
    steps = 20
    for k in range(steps):
        obs, rew, done, info = B.step(acts[k % 8].clone())
        torch.cuda.synchronize()
        o, d = obs.cpu().numpy(), done.cpu().numpy() != 0
        idx = np.nonzero(d)[0].astype(np.int32)
        demo = ds.obs[rng.randint(0, len(ds.obs), n)]
        R.imitation_reward(kind, demo, o, beta=0.7)
        if len(idx):
            pick = rng.randint(0, ds.total_T, len(idx))
            st = (EnvState * len(idx)).from_buffer_copy(states[pick].tobytes())
            bx = (BoxState * len(idx)).from_buffer_copy(ds.boxes[pick].tobytes()) if ds.boxes is not None else None
            B.set_states(idx, st, bx)
    print("%s host route (step + D2H + numpy reward + set_states of the finished envs): %.2f ms per step over %d steps" % (env_id, 1e3 * (time.perf_counter() - t0) / steps, steps))
B.close()
