"""PCIe-inclusive rate of the numpy HipVecEnv path (H2D actions, D2H packed outputs, 4096 info dicts per step).
--imitation: PickPlaceHumanCart with the action-based expert imitation reward, the device path (expert + reward in two kernels around the step kernel)
against the host route (a per-env Python expert over the materialised `previous_expert_observation` infos + the reward mix in numpy)."""
import os, sys, time, numpy as np
sys.path.insert(0, '.')
from human_robot_gym_amd.vec_env import HipVecEnv
N = 4096


def rate(env, acts, after_step=None, warm=20, steps=60):
    env.reset()
    for k in range(warm):
        out = env.step(acts[k % 8])
        if after_step: after_step(acts[k % 8], *out)
    t = time.perf_counter()
    for k in range(steps):
        out = env.step(acts[k % 8])
        if after_step: after_step(acts[k % 8], *out)
    el = time.perf_counter() - t
    env.close()
    return N * steps / el, 1e3 * el / steps


if "--imitation" in sys.argv:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import expert_ref as R
    from human_robot_gym_amd.mixed import task_clips
    pp = dict(hover_dist=0.2, tan_theta=0.5, horizontal_epsilon=0.035, vertical_epsilon=0.015, goal_dist=0.08, gripper_fully_opened_threshold=0.02, release_when_delivered=True)
    rw = dict(alpha=0.25, beta=0.7, iota_m=0.1, iota_g=0.5, m_sim_fn="gaussian", g_sim_fn="gaussian")
    keys = ["object_gripped", "vec_eef_to_object", "vec_eef_to_target", "robot0_gripper_qpos"]
    common = dict(env_id="PickPlaceHumanCart", env_kwargs=dict(shield_type="SSM", horizon=100, seed=1234), clips=task_clips("PickPlaceHumanCart", 13),
                  ik_position_delta=dict(action_limit=0.1))
    rng = np.random.RandomState(0)
    acts = [rng.uniform([-0.1] * 3 + [-1], [0.1] * 3 + [1], (N, 4)) for _ in range(8)]
    print("plain step (no imitation reward): %.0f env steps/s (%.2f ms per %d-env step)" % (*rate(HipVecEnv(N, **common), acts), N))
    print("device path (expert=, imitation_reward=): %.0f env steps/s (%.2f ms per %d-env step)"
          % (*rate(HipVecEnv(N, expert=dict(id="PickPlaceHumanCart", signal_to_noise_ratio=1.0, **pp), imitation_reward=rw, **common), acts), N))

    def host_route(a, obs, rew, done, infos):   # what a user does without the device path: one expert call per env on its info dict, then the reward mix
        x = np.empty((N, 4))
        for i, info in enumerate(infos):
            o = info["previous_expert_observation"]
            x[i] = R.pick_place(o["object_gripped"] != 0, o["vec_eef_to_object"][None], o["vec_eef_to_target"][None], o["robot0_gripper_qpos"][None], 0.1, 1.0, **pp)[0]
        r_im, _, _ = R.imitation_reward(a, x, rw["beta"], rw["iota_m"], rw["iota_g"])
        return R.combine(r_im, rew, rw["alpha"])
    print("host route (expert_obs_keys + per-env Python expert): %.0f env steps/s (%.2f ms per %d-env step)"
          % (*rate(HipVecEnv(N, expert_obs_keys=keys, **common), acts, host_route, warm=3, steps=10), N))
    sys.exit(0)

kw = dict(shield_type="SSM", control_freq=10, horizon=100, done_at_success=True, reward_shaping=True, seed=1234)
for dicts in (False, True):
    rng = np.random.RandomState(0)
    acts = [rng.uniform(-1, 1, (N, 7)) for _ in range(8)]
    r, ms = rate(HipVecEnv(N, env_kwargs=kw, info_dicts=dicts), acts)
    print("HipVecEnv numpy path, info dicts %s: %.0f env steps/s (%.2f ms per 4096-env step)" % (dicts, r, ms))
