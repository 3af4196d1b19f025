#!/usr/bin/env python3
"""Record a demonstration dataset with a scripted expert on the batched stepper (the reference's training/create_expert_dataset.py):

  python tools/create_expert_dataset.py --env PickPlaceHumanCart --name pp-demo --episodes 100 [--envs 64] [--snr 0.98] [--seed 0] [--horizon 1000]
                                        [--shield SSM|PFL|OFF] [--geometry capsule|hull] [--done-at-success true|false] [--expert-arg board_size=[1.0,0.4,0.03] ...]

writes datasets/<name>/hrg_dataset.npz (+ observations.csv, stats.csv) below the working directory, where
wrappers.state_based_expert_imitation_reward / action_based_expert_imitation_reward (dataset_name: <name>) and wrappers.dataset_obs_norm find it.
The expert is the one that carries the task's name (PickPlaceHumanCart's for the handover tasks); the Cartesian tasks are stepped through the IK front-end."""
import argparse
import ast
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from human_robot_gym_amd.dataset import DEFAULT_CAPACITY_BYTES, collect_expert_dataset, dataset_path  # noqa: E402
from human_robot_gym_amd.expert import EXPERT_ENVS  # noqa: E402
from human_robot_gym_amd.mixed import task_clips, task_env_kwargs  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--env", required=True)
    ap.add_argument("--name", required=True, help="dataset_name")
    ap.add_argument("--episodes", type=int, required=True)
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--snr", type=float, default=1.0, help="signal_to_noise_ratio of the expert")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--horizon", type=int, default=None)
    ap.add_argument("--shield", default="SSM")
    ap.add_argument("--geometry", default="capsule")
    ap.add_argument("--done-at-success", choices=["true", "false"], default=None, help="environment.done_at_success (default: the task's; the reference's data-collection "
                    "configs set it, e.g. reach_human_cart_expert_data_collection.yaml: false)")
    ap.add_argument("--action-limit", type=float, default=0.1, help="ik_position_delta.action_limit of the Cartesian tasks")
    ap.add_argument("--capacity-gib", type=float, default=DEFAULT_CAPACITY_BYTES / 2 ** 30, help="device memory the tape may take")
    ap.add_argument("--expert-arg", action="append", default=[], metavar="KEY=VALUE", help="further constructor arguments of the expert (Python literals)")
    a = ap.parse_args()
    eid = next((k for k, envs in EXPERT_ENVS.items() if a.env in envs), None)
    if eid is None:
        sys.exit(f"--env {a.env}: no scripted expert reads this task's observation ({sorted(e for v in EXPERT_ENVS.values() for e in v)})")
    expert = dict(id=eid, signal_to_noise_ratio=a.snr, seed=a.seed)
    for kv in a.expert_arg:
        k, v = kv.split("=", 1)
        expert[k] = ast.literal_eval(v)
    kw = dict(shield_type=a.shield, seed=a.seed, **task_env_kwargs(a.env))
    if a.horizon is not None:
        kw["horizon"] = a.horizon
    if a.done_at_success is not None:
        kw["done_at_success"] = a.done_at_success == "true"
    ds = collect_expert_dataset(a.env, a.episodes, a.envs, expert=expert, dataset_name=a.name, capacity_bytes=int(a.capacity_gib * 2 ** 30), env_kwargs=kw,
                                clips=task_clips(a.env), robot_geometry=a.geometry, ik_position_delta=None if a.env == "ReachHuman" else dict(action_limit=a.action_limit))
    import numpy as np
    lens = np.diff(ds.ep_offset)
    print(f"wrote {dataset_path(a.name)}: {ds.n_episodes} episodes, {ds.total_T} transitions; success rate {ds.ep_success.mean():.3f}, "
          f"episode length {lens.mean():.1f} +- {lens.std():.1f}, return {ds.ep_return.mean():.3f}")


if __name__ == "__main__":
    main()
