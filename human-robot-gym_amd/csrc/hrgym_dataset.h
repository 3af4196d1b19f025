// hrgym_dataset.h -- demonstration datasets on the device: DatasetRSIWrapper (wrappers/dataset_wrapper.py:88-157) and the three
// StateBasedExpertImitationRewardWrapper subclasses (wrappers/state_based_expert_imitation_reward_wrapper.py), batched: two small kernels behind the
// (unchanged) step launch.  Included into the base translation unit only (hrgym_hip.hip, HRG_BASE_TU), after hrgym_expert.h (expert_similarity, EXO_*).
//
//   hrg_sir_post_kernel          DatasetRSIWrapper.step's cursor (149) + _get_imitation_reward / _should_terminate_early of the wrapper that fits the task +
//                                step() 132-174: reward <- r_im alpha + r_env (1 - alpha), early termination, the per-episode sums of _add_reward_to_info,
//                                one f32 row per env.  One thread per env, 256-thread blocks, FP64 arithmetic on the f32 rows (4 - 12 floats of each).
//   hrg_dataset_restore_kernel   DatasetRSIWrapper.reset (115-135) for the envs that finished: draw (episode, start step), copy the state block, the box block
//                                and the observation row from the dataset.  One wavefront per env; a wave whose env did not finish returns at once.
//
// Draws: rng_u01 keyed by (dataset seed, global env id, the env's reset counter, STREAM_DATASET, 0..2): independent of the sharding, and no stream of the
// step / reset / expert kernels moves.  The reference draws from the global numpy stream (np.random.randint / rand, 122, 154-155).
#pragma once

enum { STREAM_DATASET = 9 };   // after STREAM_EXPERT = 8 (hrgym_expert.h)
#define HRG_DATASET_BLOCK 256
enum { HRG_FIN_DONE = 1 /* the step kernel finished the env (and auto-reset it) */, HRG_FIN_EARLY = 2 /* early termination fired */ };

// the uploaded dataset + per-env buffers of hrg_batch_dataset_attach; passed to both kernels by value
struct DatasetDev {
  const int64_t* ep_offset = nullptr;    // [n_ep + 1]
  const hrg_env_state* states = nullptr; // [total_T]
  const hrg_box_state* boxes = nullptr;  // [total_T] or null (ReachHuman)
  const float* obs = nullptr;            // [total_T + n_ep][HRG_OBS_DIM]
  int32_t* cursor = nullptr;             // [n][3] episode, step, T
  int32_t* resets = nullptr;             // [n] restores so far (key of the draws)
  double* acc = nullptr;                 // [n][6] episode sums of r_im, r_env, r_motion, r_gripper; steps; steps in the motion / gripper sums
  uint8_t* finished = nullptr;           // [n] HRG_FIN_*
  int64_t n_ep = 0, total_T = 0;
};

// 16 bytes per lane; the blocks sit at 8-byte boundaries (sizeof(hrg_box_state) is an odd multiple of 8), so the type promises no more than that
typedef uint32_t ds_u32x4 __attribute__((ext_vector_type(4), aligned(8)));

// the whole wave copies `bytes` (a multiple of 8) from src to dst: lane i moves chunk i, i + 64, ...; an 8-byte tail goes with one lane
DI void dataset_wave_copy(void* __restrict__ dst, const void* __restrict__ src, size_t bytes, int lane) {
  const size_t n16 = bytes / 16;
  const ds_u32x4* s = (const ds_u32x4*)src;
  ds_u32x4* d = (ds_u32x4*)dst;
  for (size_t i = (size_t)lane; i < n16; i += 64) d[i] = s[i];
  if ((bytes & 8) && lane == 0) ((uint64_t*)dst)[2 * n16] = ((const uint64_t*)src)[2 * n16];
}

__global__ __launch_bounds__(HRG_DATASET_BLOCK) void hrg_sir_post_kernel(const hrg_dataset_desc p, const DatasetDev ds, const float* __restrict__ obs,
                                                                         const float* __restrict__ term_obs, float* __restrict__ reward, uint8_t* __restrict__ done,
                                                                         float* __restrict__ sir, int n_envs) {
  const int e = (int)(blockIdx.x * HRG_DATASET_BLOCK + threadIdx.x);
  if (e >= n_envs) return;
  int32_t* cur = ds.cursor + 3 * (size_t)e;
  const int ep = cur[0], T = cur[2];
  const int step = min(cur[1] + 1, T);   // dataset_wrapper.py:149
  cur[1] = step;
  const bool dn = done[e] != 0;
  float* row = sir + (size_t)e * HRG_SIR_DIM;
  if (p.sir_kind == HRG_SIR_NONE) {
    ds.finished[e] = dn ? HRG_FIN_DONE : 0;
    row[HRG_SIR_TIME] = row[HRG_SIR_TIME_OBS] = (float)((double)step / (double)T);
    return;
  }
  // the state the agent reached: the terminal observation where the step kernel finished (and auto-reset) the env
  const float* o = (dn ? term_obs : obs) + (size_t)e * HRG_OBS_DIM;
  const float* dm = ds.obs + (size_t)(ds.ep_offset[ep] + ep + step) * HRG_OBS_DIM;   // _dic["expert_observations"][_dataset_ep_step_idx] (135)
  double r_im = 0.0, r_motion = 0.0, r_gripper = 0.0, dist;
  bool counted = false, early;
  if (p.sir_kind == HRG_SIR_REACH) {   // 361-413
    double d2 = 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) { const double d = (double)dm[EXO_GOAL_DIFF + k] - (double)o[EXO_GOAL_DIFF + k]; d2 += d * d; }
    dist = sqrt(d2);
    r_im = expert_similarity(p.m_sim_fn, dist, p.iota_m);
    early = dist > p.et_dist * p.iota_m;
  } else {
    const bool mismatch = dm[EXO_GRIPPED] != 0.0f && !(o[EXO_GRIPPED] != 0.0f);   // the demonstration has gripped, the agent has not
    const int c0 = p.sir_kind == HRG_SIR_PICK_PLACE ? EXO_TO_TARGET : EXO_TO_HUMAN_LH;
    double d2 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) { const double d = (double)dm[c0 + k] - (double)o[c0 + k]; d2 += d * d; }
    dist = sqrt(d2);
    if (p.sir_kind == HRG_SIR_PICK_PLACE) {   // 542-619
      if (!mismatch) {
        const double g0 = (double)dm[EXO_GRIPPER_QPOS] - (double)o[EXO_GRIPPER_QPOS], g1 = (double)dm[EXO_GRIPPER_QPOS + 1] - (double)o[EXO_GRIPPER_QPOS + 1];
        r_motion = expert_similarity(p.m_sim_fn, dist, p.iota_m);
        r_gripper = expert_similarity(p.g_sim_fn, fabs(g0 - g1), p.iota_g);
        r_im = r_motion * p.beta + r_gripper * (1.0 - p.beta);
        counted = true;
      }
      early = (mismatch && dist > p.et_dist * 0.1 * p.iota_m) || dist > p.et_dist * p.iota_m;
    } else {   // 698-758
      if (!mismatch) r_im = expert_similarity(p.m_sim_fn, dist, p.iota_m);
      early = mismatch || dist > p.et_dist * p.iota_m;
    }
  }
  early = early && p.use_et != 0;
  const double r_env = (double)reward[e];
  const double full = r_im * p.alpha + r_env * (1.0 - p.alpha);
  double* ac = ds.acc + 6 * (size_t)e;   // the restore kernel restarts them where the env finished
  const double s_im = ac[0] + r_im, s_env = ac[1] + r_env, s_m = ac[2] + r_motion, s_g = ac[3] + r_gripper, len = ac[4] + 1.0, len_mg = ac[5] + (counted ? 1.0 : 0.0);
  ac[0] = s_im; ac[1] = s_env; ac[2] = s_m; ac[3] = s_g; ac[4] = len; ac[5] = len_mg;
  row[HRG_SIR_R_IM] = (float)r_im;
  row[HRG_SIR_R_ENV] = (float)r_env;
  row[HRG_SIR_R_MOTION] = (float)r_motion;
  row[HRG_SIR_R_GRIPPER] = (float)r_gripper;
  row[HRG_SIR_R_FULL] = (float)full;
  row[HRG_SIR_EP_IM] = (float)s_im;
  row[HRG_SIR_EP_ENV] = (float)s_env;
  row[HRG_SIR_EP_MOTION] = (float)s_m;
  row[HRG_SIR_EP_GRIPPER] = (float)s_g;
  row[HRG_SIR_EP_LEN] = (float)len;
  row[HRG_SIR_EP_LEN_MG] = (float)len_mg;
  row[HRG_SIR_EARLY] = early ? 1.0f : 0.0f;
  row[HRG_SIR_TIME] = row[HRG_SIR_TIME_OBS] = (float)((double)step / (double)T);
  reward[e] = (float)full;
  ds.finished[e] = (uint8_t)((dn ? HRG_FIN_DONE : 0) | (early ? HRG_FIN_EARLY : 0));
  if (early) done[e] = 1;
}

// grid = n_envs blocks of one wavefront.  `fin`: ds.finished after a step, the caller's reset mask (null: every env) in hrg_batch_dataset_reset.
__global__ __launch_bounds__(64) void hrg_dataset_restore_kernel(const hrg_dataset_desc p, const DatasetDev ds, const uint8_t* __restrict__ fin,
                                                                 hrg_env_state* __restrict__ states, hrg_box_state* __restrict__ boxes, float* __restrict__ obs,
                                                                 float* __restrict__ term_obs, float* __restrict__ sir, int64_t env_id0, int n_envs) {
  const int e = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (e >= n_envs) return;
  const int f = fin ? (int)fin[e] : HRG_FIN_DONE;
  if (!f) return;
  float* orow = obs + (size_t)e * HRG_OBS_DIM;
  if (term_obs && f == HRG_FIN_EARLY) term_obs[(size_t)e * HRG_OBS_DIM + lane] = orow[lane];   // early termination alone: the step's observation is the terminal one
  const uint64_t gid = (uint64_t)(env_id0 + e), cnt = (uint64_t)ds.resets[e];
  const double u0 = rng_u01(p.seed, gid, cnt, STREAM_DATASET, 0), u1 = rng_u01(p.seed, gid, cnt, STREAM_DATASET, 1), u2 = rng_u01(p.seed, gid, cnt, STREAM_DATASET, 2);
  const int64_t ep = min((int64_t)floor(u0 * (double)ds.n_ep), ds.n_ep - 1);                    // np.random.randint(len(self.dataset)), 122
  const int64_t off = ds.ep_offset[ep], T = ds.ep_offset[ep + 1] - off;
  const int64_t step = u1 < p.rsi_prob ? min((int64_t)floor(u2 * (double)T), T - 1) : 0;        // _get_initial_dataset_ep_step_idx, 153-157
  dataset_wave_copy(states + e, ds.states + (off + step), sizeof(hrg_env_state), lane);
  if (ds.boxes) dataset_wave_copy(boxes + e, ds.boxes + (off + step), sizeof(hrg_box_state), lane);
  orow[lane] = ds.obs[(size_t)(off + ep + step) * HRG_OBS_DIM + lane];                          // return self._dic["observations"][idx], 135
  if (lane == 0) {
    int32_t* cur = ds.cursor + 3 * (size_t)e;
    cur[0] = (int32_t)ep; cur[1] = (int32_t)step; cur[2] = (int32_t)T;
    ds.resets[e] = (int32_t)(cnt + 1);
    if (sir) sir[(size_t)e * HRG_SIR_DIM + HRG_SIR_TIME_OBS] = (float)((double)step / (double)T);   // reset(), 107: the new episode's time
  }
  if (lane < 6) ds.acc[6 * (size_t)e + lane] = 0.0;
}
