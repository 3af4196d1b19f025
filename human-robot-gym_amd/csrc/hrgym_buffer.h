// hrgym_buffer.h -- what the device training buffers share (hrgym_her.h, hrgym_rollout.h, hrgym_replay.h): the policy's view of a row of the observation
// superset, the episode tracker behind Monitor's statistics, and the grid shape of the one-wavefront-per-row kernels.  Included into the base translation unit
// only (hrgym_hip.hip, HRG_BASE_TU), ahead of hrgym_her.h.  No LDS, no atomics, no random draws.
//
//   hrg_buffer_view_kernel   rows of the observation superset (+ a time value per row) -> the policy's view; one wavefront per row, lane k computes value k.
//                            Behind hrg_rollout_view and hrg_replay_view.
//
// The view.  Lane k < n_obs_cols takes column obs_cols[k] of the row, lane n_obs_cols the time value (observe_time); with `normalize`, (v - mean[k]) / std[k] in
// double, tanh(squash_factor * .) with `squash`, rounded to float32 once (HipVecEnv._view).  The translation unit is compiled with -fapprox-func: the double
// division is the reciprocal refinement, within an ulp of the quotient in double, so that the float32 result differs from numpy's only where the exact value
// sits next to a rounding boundary.  Without `normalize` (the rollout buffer, HER) the values are bit copies.
//
// The tracker.  Per env: the row the next transition starts from, the return and length of the running episode, and sums over the finished episodes since the
// last clear -- column 0 episodes, 1 returns, 2 lengths, 3 .. the info columns of the episodes' last steps, then what the buffer adds.  Each buffer keeps its
// own storage, slot bookkeeping and whatever else it holds per env (the rollout buffer's episode_start flag, the replay buffer's time value).
#pragma once

#define HRG_BUFFER_BLOCK 256   // four wavefronts: a row, sample or index each (or 256 envs, a lane each)

// the row / sample / index of this wavefront in a grid of ceil(n / 4) blocks of HRG_BUFFER_BLOCK threads (wave-uniform)
DI int buffer_wave_item() { return (int)(blockIdx.x * (HRG_BUFFER_BLOCK / 64) + (threadIdx.x >> 6)); }

// how the policy sees a row; passed to the kernels by value.  The tables are per-lane lookups: device memory, not kernel arguments.
struct BufferView {
  const int32_t* obs_cols = nullptr;   // [HRG_OBS_DIM] the descriptor's obs_cols, zero behind n_obs_cols
  const double* mean = nullptr;        // [HRG_OBS_DIM] zero behind K = n_obs_cols + observe_time (null without normalize)
  const double* std = nullptr;         // [HRG_OBS_DIM] one behind K (null without normalize)
  double squash_factor = 0.0;
  int32_t n_obs_cols = 0, observe_time = 0, normalize = 0, squash = 0;
};

// column obs_cols[lane] of the row whose column `lane` is x.  Every lane of the wave takes part (the shuffle).
DI float view_select(const BufferView& w, float x, int lane) { return __shfl(x, w.obs_cols[lane]); }

// value `lane` of the policy's view of a row: x = column `lane` of the row, t = its time value.  Every lane of the wave takes part.
DI float replay_view(const BufferView& w, float x, float t, int lane) {
  float v = view_select(w, x, lane);
  if (w.observe_time && lane == w.n_obs_cols) v = t;
  if (w.normalize) {
    double d = ((double)v - w.mean[lane]) / w.std[lane];
    if (w.squash) d = tanh(w.squash_factor * d);
    v = (float)d;
  }
  return v;
}

// grid = ceil(n_rows / 4) blocks of four wavefronts, one row each; time may be null without observe_time
__global__ __launch_bounds__(HRG_BUFFER_BLOCK) void hrg_buffer_view_kernel(const BufferView w, const float* __restrict__ rows, const float* __restrict__ time, int n_rows,
                                                                           float* __restrict__ out) {
  const int lane = (int)(threadIdx.x & 63);
  const int r = buffer_wave_item();
  if (r >= n_rows) return;   // (wave-uniform)
  const int K = w.n_obs_cols + w.observe_time;
  const float v = replay_view(w, rows[(size_t)r * HRG_OBS_DIM + lane], w.observe_time ? time[r] : 0.0f, lane);
  if (lane < K) out[(size_t)r * K + lane] = v;
}

// the episode bookkeeping of one buffer; part of its device struct
struct EpisodeTracker {
  float* cur_obs = nullptr;    // [n][HRG_OBS_DIM] the row the next transition starts from (SB3's _last_obs, as a row of the superset)
  double* run_ret = nullptr;   // [n] return of the running episode (Monitor's sum)
  int32_t* run_len = nullptr;  // [n] its length
  double* acc = nullptr;       // [n][the buffer's stats columns] sums over the finished episodes since the last clear
};

// env e starts an episode from row `obs` (after a reset); called by the whole wave, lane l moves column l
DI void tracker_start(const EpisodeTracker& k, int e, int lane, const float* __restrict__ obs) {
  k.cur_obs[(size_t)e * HRG_OBS_DIM + lane] = obs[(size_t)e * HRG_OBS_DIM + lane];
  if (lane == 0) {
    k.run_ret[e] = 0.0;
    k.run_len[e] = 0;
  }
}

// one step of env e; called by the whole wave.  r: the reward that feeds Monitor's return; info: the env's info row; n_cols: the buffer's stats columns, the
// last of them `extra` where there are more than 3 + HRG_INFO_DIM.  Lane 0 keeps the running return and length; on a done step lane j adds column j.
DI void tracker_step(const EpisodeTracker& k, int e, int lane, float r, bool dn, const int32_t* __restrict__ info, int n_cols, double extra) {
  const double ep_ret = k.run_ret[e] + (double)r;   // (the same value on every lane)
  const int32_t ep_len = k.run_len[e] + 1;
  if (lane == 0) {
    k.run_ret[e] = dn ? 0.0 : ep_ret;
    k.run_len[e] = dn ? 0 : ep_len;
  }
  if (dn && lane < n_cols) {
    const double x = lane == 0 ? 1.0 : lane == 1 ? ep_ret : lane == 2 ? (double)ep_len : lane < 3 + HRG_INFO_DIM ? (double)info[lane - 3] : extra;
    k.acc[(size_t)e * n_cols + lane] += x;
  }
}
