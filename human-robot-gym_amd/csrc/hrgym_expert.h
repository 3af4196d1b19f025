// hrgym_expert.h -- the scripted experts of demonstrations/experts/ and ActionBasedExpertImitationRewardWrapper, batched: two small kernels around the
// (unchanged) step launch.  Included into the base translation unit only (hrgym_hip.hip, HRG_BASE_TU).
//
//   hrg_expert_pre_kernel       Expert.__call__ on the observation the policy acted on (info["previous_expert_observation"]: obs_dev as the previous step / reset left
//                               it) + the two similarities against the agent's action rows, read BEFORE the step kernel rewrites them (IK front-end, collision
//                               prevention).  With agent == nullptr: the expert's actions alone (hrg_batch_expert_actions, dataset collection).
//   hrg_imitation_post_kernel   reward <- r_im alpha + r_env (1 - alpha), the per-episode sums of _add_reward_to_info, one f32 row per env.
//
// One thread per env, 256-thread blocks, no LDS; FP64 arithmetic on the f32 observation row, of which a thread reads only the columns its expert needs
// (4 - 9 floats of the 64).  Both kernels are a few hundred bytes of traffic per env: their cost is their launch.
//
// Noise: the experts' ReparameterizedOrnsteinUhlenbeckProcess (utils/ou_process.py), y <- y + alpha (mu - y) dt + sigma sqrt(2 alpha) sqrt(dt) xi, one state
// vector and one call counter per env in batch buffers; like the reference's expert object it is never reset at episode ends.  xi = rng_gauss keyed by (expert
// seed, global env id, 0, STREAM_EXPERT, call counter x dim + k): independent of the sharding, and no stream of the step / reset kernels moves.
#pragma once

enum { STREAM_EXPERT = 8 };   // after STREAM_LOOP = 7 (hrgym_device.h)
#define HRG_EXPERT_BLOCK 256
#define HRG_EXPERT_TAN_HALF 0.5463024898437905   // tan(0.5), expert_imitation_reward_utils.py:48
// observation columns the experts read (include/hrgym.h HRG_OBS_DIM; vec_env.OBS_COLUMNS / OBS_COLUMNS_TASK)
enum { EXO_GOAL_DIFF = 12, EXO_GRIPPED = 39, EXO_TO_OBJECT = 40, EXO_TO_TARGET = 43, EXO_GRIPPER_QPOS = 53, EXO_TO_HUMAN_LH = 0, EXO_TO_HUMAN_RH = 4, EXO_TO_NAIL = 43 };

// per-env buffers of an attached expert (hrg_batch_expert_attach)
struct ExpertBuffers {
  double* act = nullptr;      // [n][HRG_ACT_DIM] the expert's action of the last pre kernel
  double* sim = nullptr;      // [n][2] r_motion, r_gripper
  double* ou_y = nullptr;     // [n][HRG_ACT_DIM] noise state
  int64_t* ou_calls = nullptr; // [n] noise steps taken
  double* acc = nullptr;      // [n][3] episode sums of r_im, r_env; episode length
};

DI double expert_clip(double x, double lo, double hi) { return fmin(fmax(x, lo), hi); }   // np.clip

// one step of the env's noise process: y (registers) and the batch buffers advance together
template <int DIM>
DI void expert_ou_step(const hrg_expert_desc& p, double alpha, double sigma, int64_t gid, double* __restrict__ y_row, int64_t* __restrict__ calls, double* y) {
  const int64_t c = *calls;
  const double dt = p.delta_time, amp = sigma * sqrt(2.0 * alpha) * sqrt(dt);
#pragma unroll
  for (int k = 0; k < DIM; k++) {
    const double xi = rng_gauss(p.seed, (uint64_t)gid, 0, STREAM_EXPERT, (uint64_t)(c * DIM + k)), y0 = y_row[k];
    y[k] = y0 + (alpha * (0.0 - y0) * dt + amp * xi);
    y_row[k] = y[k];
  }
  *calls = c + 1;
}

// ReachHumanExpert.__call__ (reach_human_expert.py:79-90): the joints move straight to their goal angles; the noise is scaled to half the action range
DI void expert_reach(const hrg_expert_desc& p, const float* __restrict__ o, const double* y, double* a) {
  const double snr = p.signal_to_noise_ratio;
#pragma unroll
  for (int k = 0; k < HRG_ACT_DIM; k++) {
    const double lo = p.act_low[k], hi = p.act_high[k];
    const double motion = expert_clip(k < HRG_NARM ? (double)o[EXO_GOAL_DIFF + k] : 0.0, lo, hi);
    a[k] = expert_clip(snr * motion + y[k] * (1.0 - snr) * 0.5 * (hi - lo), lo, hi);
  }
}

// PickPlaceHumanCartExpert.__call__ (pick_place_human_cart_expert.py:130-288): hover above the object with the gripper open, descend, grip, hover above the
// target, descend, release.  The noise enters the motion only.
DI void expert_pick_place(const hrg_expert_desc& p, const float* __restrict__ o, const double* y, double* a) {
  const bool gripped = o[EXO_GRIPPED] != 0.0f;
  const double obj[3] = {(double)o[EXO_TO_OBJECT], (double)o[EXO_TO_OBJECT + 1], (double)o[EXO_TO_OBJECT + 2]};
  const double tgt[3] = {(double)o[EXO_TO_TARGET], (double)o[EXO_TO_TARGET + 1], (double)o[EXO_TO_TARGET + 2]};
  const double he = p.horizontal_epsilon, ve = p.vertical_epsilon;
  const bool opened = (double)o[EXO_GRIPPER_QPOS] - (double)o[EXO_GRIPPER_QPOS + 1] > p.gripper_fully_opened_threshold;
  const double o2t[3] = {tgt[0] - obj[0], tgt[1] - obj[1], tgt[2] - obj[2]};
  const bool delivered = sqrt(o2t[0] * o2t[0] + o2t[1] * o2t[1]) < he && fabs(o2t[2]) < ve;
  const bool at_object = sqrt(obj[0] * obj[0] + obj[1] * obj[1]) < he && -obj[2] < ve;
  // truncated cone above the next objective: radius horizontal_epsilon at its tip, opening tan_theta, towards -z of the vector
  const bool above_object = sqrt(obj[0] * obj[0] + obj[1] * obj[1]) < he - obj[2] * p.tan_theta && obj[2] < 0.0;
  const bool above_target = sqrt(tgt[0] * tgt[0] + tgt[1] * tgt[1]) < he - tgt[2] * p.tan_theta && tgt[2] < 0.0;
  bool to_target, hover;   // _select_motion (169-189), in its branch order
  if (delivered && opened) { to_target = false; hover = true; }
  else if (above_object && opened) { to_target = false; hover = false; }
  else if (above_target && gripped) { to_target = true; hover = false; }
  else if (gripped) { to_target = true; hover = true; }
  else { to_target = false; hover = true; }
  const double lim = p.act_high[0], snr = p.signal_to_noise_ratio;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    double m = to_target ? tgt[k] : obj[k];
    if (k == 2 && hover) m += p.hover_dist;
    m = expert_clip(m, -lim, lim);
    a[k] = expert_clip(m * snr + y[k] * (1.0 - snr), -lim, lim);
  }
  // _select_gripper_action (191-206): open (-1) / close (+1)
  const double g = (delivered && p.release_when_delivered) ? -1.0 : ((gripped || at_object) ? 1.0 : -1.0);
  a[3] = expert_clip(g, -p.act_high[3], p.act_high[3]);
}

// CollaborativeLiftingCartExpert.__call__ (collaborative_lifting_cart_expert.py:98-128): follow the midpoint of the human's hands at its height, a board
// length (minus the grip offset) away; the gripper stays closed.  Motion and noise are clipped separately, their mix is not.
DI void expert_lifting(const hrg_expert_desc& p, const float* __restrict__ o, const double* y, double* a) {
  double v[3];
#pragma unroll
  for (int k = 0; k < 3; k++) v[k] = ((double)o[EXO_TO_HUMAN_LH + k] + (double)o[EXO_TO_HUMAN_RH + k]) / 2.0;
  const double nrm = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), reach = p.board_size[0] - p.human_grip_offset;
  const double lim = p.act_high[0], snr = p.signal_to_noise_ratio;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double m = expert_clip(k < 2 ? v[k] - reach * (v[k] / nrm) : v[2], -lim, lim);
    a[k] = m * snr + expert_clip(y[k], -lim, lim) * (1.0 - snr);
  }
  a[3] = p.act_high[3];
}

// CollaborativeHammeringCartExpert.__call__ (collaborative_hammering_cart_expert.py:73-91): to a point 0.1 m in front of the nail, clipped to 0.1 (both literals
// of the reference); the gripper stays closed.  Its noise process is constructed and never stepped.
DI void expert_hammering(const float* __restrict__ o, double* a) {
#pragma unroll
  for (int k = 0; k < 3; k++) a[k] = expert_clip((double)o[EXO_TO_NAIL + k] + (k == 0 ? -0.1 : 0.0), -0.1, 0.1);
  a[3] = 1.0;
}

// ReachHumanCartExpert.__call__ (reach_human_cart_expert.py:70-87): the end effector moves straight to the goal position (goal_difference[0:3]); gripper action 0
DI void expert_reach_cart(const hrg_expert_desc& p, const float* __restrict__ o, const double* y, double* a) {
  const double lim = p.act_high[0], snr = p.signal_to_noise_ratio;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double m = expert_clip((double)o[EXO_GOAL_DIFF + k], -lim, lim);
    a[k] = expert_clip(snr * m + y[k] * (1.0 - snr), -lim, lim);
  }
  a[3] = 0.0;
}

// similarity_fn (utils/expert_imitation_reward_utils.py:51-73)
DI double expert_similarity(int fn, double delta, double iota) {
  if (fn == HRG_SIM_TANH) return -tanh(HRG_EXPERT_TAN_HALF * delta / iota) + 1.0;
  const double x = delta / iota;
  return exp2(-(x * x));
}

__global__ __launch_bounds__(HRG_EXPERT_BLOCK) void hrg_expert_pre_kernel(const hrg_expert_desc p, const float* __restrict__ obs, const double* __restrict__ agent,
                                                                          double* __restrict__ act_out, double* __restrict__ sim, double* __restrict__ ou_y,
                                                                          int64_t* __restrict__ ou_calls, int64_t env_id0, int n_envs) {
  const int e = (int)(blockIdx.x * HRG_EXPERT_BLOCK + threadIdx.x);
  if (e >= n_envs) return;
  const float* o = obs + (size_t)e * HRG_OBS_DIM;
  double* yrow = ou_y + (size_t)e * HRG_ACT_DIM;
  const int64_t gid = env_id0 + e;
  double a[HRG_ACT_DIM] = {0, 0, 0, 0, 0, 0, 0}, y[HRG_ACT_DIM] = {0, 0, 0, 0, 0, 0, 0};
  if (p.expert == HRG_EXPERT_REACH) {
    expert_ou_step<HRG_ACT_DIM>(p, 10.0, 0.5, gid, yrow, ou_calls + e, y);
    expert_reach(p, o, y, a);
  } else if (p.expert == HRG_EXPERT_HAMMERING) {
    expert_hammering(o, a);
  } else {
    expert_ou_step<3>(p, 0.5, p.act_high[0] * 0.5, gid, yrow, ou_calls + e, y);
    if (p.expert == HRG_EXPERT_PICK_PLACE) expert_pick_place(p, o, y, a);
    else if (p.expert == HRG_EXPERT_REACH_CART) expert_reach_cart(p, o, y, a);
    else expert_lifting(p, o, y, a);
  }
  double* out = act_out + (size_t)e * HRG_ACT_DIM;
#pragma unroll
  for (int k = 0; k < HRG_ACT_DIM; k++) out[k] = a[k];
  if (!agent) return;
  // get_imitation_reward (Cart form 365-395, Joint form 249-301): distance of the motion parts, distance of the gripper parts
  const double* ag = agent + (size_t)e * HRG_ACT_DIM;
  double d2 = 0.0, dg;
  if (p.cartesian) {
#pragma unroll
    for (int k = 0; k < 3; k++) { const double d = ag[k] - a[k]; d2 += d * d; }
    dg = fabs(ag[3] - a[3]);
  } else {
#pragma unroll
    for (int k = 0; k < HRG_ACT_DIM - 1; k++) {
      double x = ag[k], z = a[k];
      if (p.normalize_joint_actions) {
        const double lo = p.act_low[k], w = p.act_high[k] - lo;
        x = 2.0 * (x - lo) / w - 1.0;
        z = 2.0 * (z - lo) / w - 1.0;
      }
      const double d = x - z;
      d2 += d * d;
    }
    dg = fabs(ag[HRG_ACT_DIM - 1] - a[HRG_ACT_DIM - 1]);
  }
  sim[2 * (size_t)e] = expert_similarity(p.m_sim_fn, sqrt(d2), p.iota_m);
  sim[2 * (size_t)e + 1] = expert_similarity(p.g_sim_fn, dg, p.iota_g);
}

// ActionBasedExpertImitationRewardWrapper.step (96-105) after the env's step: reward_dev holds r_env
__global__ __launch_bounds__(HRG_EXPERT_BLOCK) void hrg_imitation_post_kernel(const hrg_expert_desc p, const double* __restrict__ sim, const uint8_t* __restrict__ done,
                                                                              float* __restrict__ reward, double* __restrict__ acc, float* __restrict__ imit, int n_envs) {
  const int e = (int)(blockIdx.x * HRG_EXPERT_BLOCK + threadIdx.x);
  if (e >= n_envs) return;
  const double r_motion = sim[2 * (size_t)e], r_gripper = sim[2 * (size_t)e + 1];
  const double r_im = r_motion * p.beta + r_gripper * (1.0 - p.beta);
  const double r_env = (double)reward[e];
  const double full = r_im * p.alpha + r_env * (1.0 - p.alpha);
  double* ac = acc + 3 * (size_t)e;
  const double s_im = ac[0] + r_im, s_env = ac[1] + r_env, len = ac[2] + 1.0;
  const bool fin = done[e] != 0;
  ac[0] = fin ? 0.0 : s_im;
  ac[1] = fin ? 0.0 : s_env;
  ac[2] = fin ? 0.0 : len;
  float* row = imit + (size_t)e * HRG_IMIT_DIM;
  row[HRG_IMIT_R_IM] = (float)r_im;
  row[HRG_IMIT_R_ENV] = (float)r_env;
  row[HRG_IMIT_R_MOTION] = (float)r_motion;
  row[HRG_IMIT_R_GRIPPER] = (float)r_gripper;
  row[HRG_IMIT_EP_IM] = (float)s_im;
  row[HRG_IMIT_EP_ENV] = (float)s_env;
  row[HRG_IMIT_EP_LEN] = (float)len;
  row[HRG_IMIT_R_FULL] = (float)full;
  reward[e] = (float)full;
}
