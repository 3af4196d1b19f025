"""How many of 64 PickPlaceHumanCart episodes the scripted expert completes on the stand-in gripper: 64 envs, each env's FIRST episode, driven by
env.expert_actions() (signal_to_noise_ratio 1, the PP-AIR expert parameters and wrappers, horizon 1000, done_at_success).  Report only.
python tools/expert_episodes.py"""
import sys
import numpy as np
sys.path.insert(0, '.')
from human_robot_gym_amd.vec_env import HipVecEnv
from human_robot_gym_amd.mixed import task_clips

n, horizon = 64, 1000
pp = dict(hover_dist=0.2, tan_theta=0.5, horizontal_epsilon=0.035, vertical_epsilon=0.015, goal_dist=0.08, gripper_fully_opened_threshold=0.02, release_when_delivered=True)
env = HipVecEnv(n, env_id="PickPlaceHumanCart", env_kwargs=dict(shield_type="SSM", horizon=horizon, done_at_success=True, goal_dist=0.1, seed=1234),
                clips=task_clips("PickPlaceHumanCart", 13), ik_position_delta=dict(action_limit=0.1), collision_prevention=dict(replace_type=0, n_resamples=20),
                expert=dict(id="PickPlaceHumanCart", signal_to_noise_ratio=1.0, **pp))
env.reset()
open_ = np.ones(n, bool)
length, success, ever_gripped = np.zeros(n, int), np.zeros(n, bool), np.zeros(n, bool)
cause = {}
for k in range(horizon):
    obs, rew, done, infos = env.step(env.expert_actions())
    ever_gripped |= open_ & (env._last_full[:, 39] != 0)
    for i in np.nonzero(done & open_)[0]:
        d = infos[i]
        open_[i] = False
        length[i] = d["episode"]["l"]
        success[i] = d["n_goal_reached"] > 0 and not d["TimeLimit.truncated"]
        why = "success" if success[i] else "time limit" if d["TimeLimit.truncated"] else "sim crash" if d["sim_crash"] else "collision" if d["collision"] else "other"
        cause[why] = cause.get(why, 0) + 1
    if not open_.any():
        break
env.close()
print("PickPlaceHumanCart, expert-driven, first episode of %d envs (horizon %d): %d completed (object delivered to the target); episode ends: %s" % (n, horizon, int(success.sum()), cause))
print("envs that gripped the object at some step of that episode: %d; mean length of the completed episodes: %s steps" % (int(ever_gripped.sum()), ("%.1f" % length[success].mean()) if success.any() else "-"))
