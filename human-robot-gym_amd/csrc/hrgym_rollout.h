// hrgym_rollout.h -- the PPO rollout buffer on the device: SB3's RolloutBuffer and the bookkeeping of OnPolicyAlgorithm.collect_rollouts (storage behind the
// step, bootstrapping of time-limit truncations, GAE(lambda), minibatch gather) plus the episode statistics Monitor and callbacks/logging_callback.py would have
// produced on the host, in four small kernels next to the (unchanged) step launch.  Included into the base translation unit only (hrgym_hip.hip, HRG_BASE_TU),
// after hrgym_her.h.  No LDS, no atomics, no random draws.  The policy's view of rows (hrg_rollout_view) is hrg_buffer_view_kernel, the episode statistics are
// the shared tracker (hrgym_buffer.h).
//
//   hrg_rollout_observe_kernel  after a reset: the current row of the masked envs, their episode_start flag, their running return and length.
//   hrg_rollout_add_kernel      collect_rollouts + RolloutBuffer.add for slot t of every env; one wavefront per env.
//   hrg_rollout_gae_kernel      compute_returns_and_advantage; one lane per env, the time loop serial from t = T - 1 down.
//   hrg_rollout_get_kernel      _get_samples: B flat indices -> observations, actions, old values, old log probs, advantages, returns; one wavefront per index.
//
// Layout.  Observation and action rows are env-major, [n][T][.]: row e * T + t is SB3's swap_and_flatten order, so a gathered sample is one contiguous row.
// The per-step scalars (reward, value, log prob, episode_start, advantage, return) are time-major, [T][n]: the add kernel's slot t and the GAE loop's step t are
// contiguous over the envs, so that a wave's loads coalesce.
//
// Arithmetic.  SB3 computes in numpy float32; the bootstrap line and the GAE recursion are written in its operation order with contraction off, so that no
// multiply-add pair becomes an FMA and the device gives the restatement's bits (tests/rollout_ref.py).
#pragma once

#define HRG_ROLLOUT_STATS_DIM (3 + HRG_INFO_DIM)   // episodes, return, length, the info columns

// the buffers of one hrg_rollout; passed to the kernels by value
struct RolloutDev {
  float* obs = nullptr;        // [n][T][n_obs_cols] the policy's view of the row before the step
  float* act = nullptr;        // [n][T][act_dim] the policy's own (unclipped) action
  float* reward = nullptr;     // [T][n] with the bootstrap term where the step was truncated
  float* value = nullptr;      // [T][n]
  float* log_prob = nullptr;   // [T][n]
  float* ep_start = nullptr;   // [T][n] 1 where slot t is the first step of an episode
  float* adv = nullptr;        // [T][n]
  float* ret = nullptr;        // [T][n]
  float* flag = nullptr;       // [n] episode_start flag of the next slot (SB3's _last_episode_starts)
  EpisodeTracker ep;           // the current rows; the returns are the step rewards without bootstrap terms; HRG_ROLLOUT_STATS_DIM columns
  BufferView view;             // hrg_rollout_desc::obs_cols (a plain selection: no time column, no normalisation)
};

// reward + gamma * terminal value as two float32 operations (collect_rollouts: rewards[idx] += self.gamma * terminal_value)
DI float rollout_bootstrap(float r, float g, float tv) {
#pragma clang fp contract(off)
  const float b = g * tv;
  return r + b;
}

// one step of compute_returns_and_advantage in numpy's float32 operation order; returns last_gae_lam
DI float rollout_gae_step(float r, float v, float nv, float nnt, float g, float gl, float last) {
#pragma clang fp contract(off)
  const float gnv = g * nv;
  const float boot = gnv * nnt;
  const float target = r + boot;
  const float delta = target - v;
  const float w = gl * nnt;
  const float carry = w * last;
  return delta + carry;
}

// grid = n_envs blocks of one wavefront; mask null: every env
__global__ __launch_bounds__(64) void hrg_rollout_observe_kernel(const hrg_rollout_desc p, const RolloutDev h, const float* __restrict__ obs,
                                                                 const uint8_t* __restrict__ mask) {
  const int e = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (e >= p.n_envs) return;
  if (mask && !mask[e]) return;
  tracker_start(h.ep, e, lane, obs);
  if (lane == 0) h.flag[e] = 1.0f;
}

// grid = n_envs blocks of one wavefront; t: the slot (0 <= t < n_steps, checked by the host); terminal_values may be null
__global__ __launch_bounds__(64) void hrg_rollout_add_kernel(const hrg_rollout_desc p, const RolloutDev h, int t, const float* __restrict__ actions,
                                                             const float* __restrict__ values, const float* __restrict__ log_probs,
                                                             const float* __restrict__ terminal_values, const float* __restrict__ obs,
                                                             const float* __restrict__ reward, const uint8_t* __restrict__ done, const int32_t* __restrict__ info) {
  const int e = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (e >= p.n_envs) return;
  const size_t row = (size_t)e * (size_t)p.n_steps + (size_t)t, s = (size_t)t * (size_t)p.n_envs + (size_t)e;
  const bool dn = done[e] != 0;
  const float v = view_select(h.view, h.ep.cur_obs[(size_t)e * HRG_OBS_DIM + lane], lane);   // every lane takes part
  if (lane < p.n_obs_cols) h.obs[row * (size_t)p.n_obs_cols + lane] = v;
  h.ep.cur_obs[(size_t)e * HRG_OBS_DIM + lane] = obs[(size_t)e * HRG_OBS_DIM + lane];   // after an auto-reset: the new episode's first row
  if (lane < p.act_dim) h.act[row * (size_t)p.act_dim + lane] = actions[(size_t)e * p.act_dim + lane];
  const float r = reward[e];
  tracker_step(h.ep, e, lane, r, dn, info + (size_t)e * HRG_INFO_DIM, HRG_ROLLOUT_STATS_DIM, 0.0);   // Monitor's return: the step reward, no bootstrap term
  if (lane == 0) {
    const bool boot = dn && terminal_values != nullptr && info[(size_t)e * HRG_INFO_DIM + HRG_INFO_TRUNCATED] != 0;
    h.reward[s] = boot ? rollout_bootstrap(r, (float)p.gamma, terminal_values[e]) : r;
    h.value[s] = values[e];
    h.log_prob[s] = log_probs[e];
    h.ep_start[s] = h.flag[e];
    h.flag[e] = dn ? 1.0f : 0.0f;
  }
}

// grid = ceil(n_envs / 256) blocks, one lane per env
__global__ __launch_bounds__(HRG_BUFFER_BLOCK) void hrg_rollout_gae_kernel(const hrg_rollout_desc p, const RolloutDev h, const float* __restrict__ last_values) {
  const int e = (int)(blockIdx.x * HRG_BUFFER_BLOCK + threadIdx.x);
  if (e >= p.n_envs) return;
  const size_t n = (size_t)p.n_envs;
  const float g = (float)p.gamma, gl = (float)(p.gamma * p.gae_lambda);   // (the product in double, as Python takes it)
  float nnt = 1.0f - h.flag[e], nv = last_values[e], last = 0.0f;
  for (int t = p.n_steps - 1; t >= 0; t--) {
    const size_t s = (size_t)t * n + (size_t)e;
    const float v = h.value[s];
    last = rollout_gae_step(h.reward[s], v, nv, nnt, g, gl, last);
    h.adv[s] = last;
    h.ret[s] = last + v;
    nnt = 1.0f - h.ep_start[s];   // what step t - 1 reads as episode_starts[t]
    nv = v;
  }
}

// grid = ceil(batch / 4) blocks of four wavefronts, one flat index (env * n_steps + step) each.  The indices are the caller's: not checked here.
__global__ __launch_bounds__(HRG_BUFFER_BLOCK) void hrg_rollout_get_kernel(const hrg_rollout_desc p, const RolloutDev h, const int64_t* __restrict__ index, int batch,
                                                                            float* __restrict__ o_obs, float* __restrict__ o_act, float* __restrict__ o_val,
                                                                            float* __restrict__ o_logp, float* __restrict__ o_adv, float* __restrict__ o_ret) {
  const int lane = (int)(threadIdx.x & 63);
  const int k = buffer_wave_item();
  if (k >= batch) return;
  const int64_t i = index[k];
  const int64_t e = i / p.n_steps, t = i - e * p.n_steps;
  const size_t s = (size_t)t * (size_t)p.n_envs + (size_t)e;
  if (lane < p.n_obs_cols) o_obs[(size_t)k * p.n_obs_cols + lane] = h.obs[(size_t)i * p.n_obs_cols + lane];
  if (lane < p.act_dim) o_act[(size_t)k * p.act_dim + lane] = h.act[(size_t)i * p.act_dim + lane];
  if (lane == 0) {
    o_val[k] = h.value[s];
    o_logp[k] = h.log_prob[s];
    o_adv[k] = h.adv[s];
    o_ret[k] = h.ret[s];
  }
}
