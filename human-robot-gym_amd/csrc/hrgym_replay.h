// hrgym_replay.h -- the uniform replay buffer of SAC on flat observations on the device: SB3's ReplayBuffer (add, sample, _get_samples with
// optimize_memory_usage = False) and the bookkeeping of OffPolicyAlgorithm._store_transition (the terminal observation as the next observation of a done step,
// _last_obs), the policy's view of a row with DatasetObsNormWrapper's normalisation and the state imitation reward's time column, plus the episode statistics
// Monitor and the imitation wrappers' _add_reward_to_info would have produced on the host, in three small kernels next to the (unchanged) step launch.  Included
// into the base translation unit only (hrgym_hip.hip, HRG_BASE_TU), after hrgym_rollout.h.  No LDS, no atomics.  The policy's view of rows (hrg_replay_view) is
// hrg_buffer_view_kernel, the view of a stored row replay_view, the episode statistics the shared tracker (hrgym_buffer.h).
//
//   hrg_replay_observe_kernel  after a reset: the current row and time value of the masked envs, their running return and length.
//   hrg_replay_add_kernel      _store_transition + ReplayBuffer.add for slot `pos` of every env; one wavefront per env.
//   hrg_replay_sample_kernel   ReplayBuffer.sample + _get_samples: B (slot, env) pairs, drawn or supplied -> observations, actions, next observations,
//                              dones * (1 - timeouts), rewards; one wavefront per sample.  With a seeds table (a SAC population's grouped sample): `groups` batches of
//                              `batch` samples, batch g from the envs of group g under seeds[g].
//
// Layout.  Everything is time-major, [capacity][n_envs][.], as SB3 keeps it: one step writes one contiguous block of each array.  Observations are stored as the
// policy sees them (selected, with the time column, normalised): K = n_obs_cols + observe_time floats, not the 64 of the superset.
//
// Draws: rng_u01 keyed by (buffer seed, sample call counter, index of the sample in its batch, STREAM_REPLAY, 0..1): independent of the grid and of the batch
// size, and no stream of the step / reset / expert / dataset / HER kernels moves.
#pragma once

enum { STREAM_REPLAY = 11 };   // after STREAM_HER = 10 (hrgym_her.h)

// one hrg_replay: its sizes and switches (from hrg_replay_desc) and its buffers; passed to the kernels by value
struct ReplayDev {
  float* obs = nullptr;         // [cap][n][K] the policy's view of the row before the step
  float* nobs = nullptr;        // [cap][n][K] ... of the row after it (the terminal observation where the step finished the env)
  float* act = nullptr;         // [cap][n][act_dim] the agent's own action at the policy's scale
  float* reward = nullptr;      // [cap][n]
  uint8_t* done = nullptr;      // [cap][n]
  uint8_t* timeout = nullptr;   // [cap][n] TimeLimit.truncated
  float* cur_time = nullptr;    // [n] the time value of the env's current row
  EpisodeTracker ep;            // the current rows; the returns are the env's own reward; HRG_REPLAY_STATS_DIM columns, the last the imitation reward sums
  BufferView view;              // hrg_replay_desc: obs_cols, observe_time, mean / std, squash
  uint64_t seed = 0;
  int32_t n_envs = 0, capacity = 0, act_dim = 0;
};

// grid = n_envs blocks of one wavefront; mask null: every env; time may be null without observe_time
__global__ __launch_bounds__(64) void hrg_replay_observe_kernel(const ReplayDev h, const float* __restrict__ obs, const float* __restrict__ time,
                                                                const uint8_t* __restrict__ mask) {
  const int e = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (e >= h.n_envs) return;
  if (mask && !mask[e]) return;
  tracker_start(h.ep, e, lane, obs);
  if (lane == 0) h.cur_time[e] = h.view.observe_time ? time[e] : 0.0f;
}

// grid = n_envs blocks of one wavefront; pos: the slot (0 <= pos < capacity, kept by the host).  imit / sir: the step's imitation rows or null (at most one of
// them; sir is there with observe_time -- the host checks both).
__global__ __launch_bounds__(64) void hrg_replay_add_kernel(const ReplayDev h, int pos, const float* __restrict__ actions, const float* __restrict__ obs,
                                                            const float* __restrict__ term_obs, const float* __restrict__ reward, const uint8_t* __restrict__ done,
                                                            const int32_t* __restrict__ info, const float* __restrict__ imit, const float* __restrict__ sir) {
  const int e = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (e >= h.n_envs) return;
  const int K = h.view.n_obs_cols + h.view.observe_time;
  const size_t s = (size_t)pos * (size_t)h.n_envs + (size_t)e;
  const bool dn = done[e] != 0;
  const float* srow = sir ? sir + (size_t)e * HRG_SIR_DIM : nullptr;
  const float* irow = imit ? imit + (size_t)e * HRG_IMIT_DIM : nullptr;
  const float t_next = h.view.observe_time ? srow[dn ? HRG_SIR_TIME : HRG_SIR_TIME_OBS] : 0.0f;   // the terminal observation carries the time after the step
  const float t_obs = h.view.observe_time ? srow[HRG_SIR_TIME_OBS] : 0.0f;
  const float o = obs[(size_t)e * HRG_OBS_DIM + lane];
  const float nx = dn ? term_obs[(size_t)e * HRG_OBS_DIM + lane] : o;
  const float v0 = replay_view(h.view, h.ep.cur_obs[(size_t)e * HRG_OBS_DIM + lane], h.cur_time[e], lane);
  const float v1 = replay_view(h.view, nx, t_next, lane);
  if (lane < K) {
    h.obs[s * (size_t)K + lane] = v0;
    h.nobs[s * (size_t)K + lane] = v1;
  }
  h.ep.cur_obs[(size_t)e * HRG_OBS_DIM + lane] = o;   // after an auto-reset: the new episode's first row
  if (lane < h.act_dim) h.act[s * (size_t)h.act_dim + lane] = actions[(size_t)e * h.act_dim + lane];
  const float r = reward[e];
  const float r_env = srow ? srow[HRG_SIR_R_ENV] : irow ? irow[HRG_IMIT_R_ENV] : r;   // Monitor sits inside the imitation wrapper: its return is the env's own reward
  const double ep_im = !dn ? 0.0 : srow ? (double)srow[HRG_SIR_EP_IM] : irow ? (double)irow[HRG_IMIT_EP_IM] : 0.0;   // the episode's sum of imitation rewards (ep_im_rew_mean)
  tracker_step(h.ep, e, lane, r_env, dn, info + (size_t)e * HRG_INFO_DIM, HRG_REPLAY_STATS_DIM, ep_im);
  if (lane == 0) {
    h.reward[s] = r;
    h.done[s] = dn ? 1 : 0;
    h.timeout[s] = info[(size_t)e * HRG_INFO_DIM + HRG_INFO_TRUNCATED] != 0 ? 1 : 0;
    h.cur_time[e] = t_obs;
  }
}

// grid = ceil(batch / 4) blocks of four wavefronts, one sample each.  upper: slots that hold a transition (>= 1, checked by the host); index_in [batch][2]
// (slot, env) or null: drawn; index_out [batch][2] or null.  Slot and env are clamped to the buffer: a supplied pair never reads outside it.
// The grouped sample: grid = ceil(groups * batch / 4), seeds [groups], n_envs a multiple of groups (checked by the host); sample k of group g is output row
// g * batch + k and draws the lone buffer's pair of (seeds[g], call, k) within the m = n_envs / groups envs of its group.  seeds null: groups = 1, the buffer's seed.
__global__ __launch_bounds__(HRG_BUFFER_BLOCK) void hrg_replay_sample_kernel(const ReplayDev h, int64_t upper, uint64_t call, const int64_t* __restrict__ index_in,
                                                                             int batch, int groups, const uint64_t* __restrict__ seeds, float* __restrict__ o_obs, float* __restrict__ o_act,
                                                                             float* __restrict__ o_nobs, float* __restrict__ o_done, float* __restrict__ o_rew,
                                                                             int64_t* __restrict__ index_out) {
  const int lane = (int)(threadIdx.x & 63);
  const int k = buffer_wave_item();
  if (k >= batch * groups) return;
  int64_t slot, env;
  if (index_in) {
    slot = index_in[2 * (size_t)k];
    env = index_in[2 * (size_t)k + 1];
  } else {   // np.random.randint(0, upper_bound), np.random.randint(0, n_envs)
    const int g = k / batch, m = h.n_envs / groups;
    const uint64_t seed = seeds ? seeds[g] : h.seed, kg = (uint64_t)(k - g * batch);
    const double u0 = rng_u01(seed, call, kg, STREAM_REPLAY, 0), u1 = rng_u01(seed, call, kg, STREAM_REPLAY, 1);
    slot = (int64_t)floor(u0 * (double)upper);
    env = (int64_t)g * m + min((int64_t)floor(u1 * (double)m), (int64_t)m - 1);   // (u1 < 1: the bound keeps a group's draw inside the group whatever the rounding)
  }
  slot = min(max(slot, (int64_t)0), min(upper, (int64_t)h.capacity) - 1);
  env = min(max(env, (int64_t)0), (int64_t)h.n_envs - 1);
  const int K = h.view.n_obs_cols + h.view.observe_time;
  const size_t s = (size_t)slot * (size_t)h.n_envs + (size_t)env;
  if (lane < K) {
    o_obs[(size_t)k * K + lane] = h.obs[s * (size_t)K + lane];
    o_nobs[(size_t)k * K + lane] = h.nobs[s * (size_t)K + lane];
  }
  if (lane < h.act_dim) o_act[(size_t)k * h.act_dim + lane] = h.act[s * (size_t)h.act_dim + lane];
  if (lane == 0) {
    o_done[k] = (h.done[s] != 0 && h.timeout[s] == 0) ? 1.0f : 0.0f;   // dones * (1 - timeouts): a timeout is no termination
    o_rew[k] = h.reward[s];
    if (index_out) { index_out[2 * (size_t)k] = slot; index_out[2 * (size_t)k + 1] = env; }
  }
}
