// hrgym_eval.h -- evaluation of deterministic policies on the device: [UPSTREAM] stable-baselines3 1.5.0 evaluate_policy (written out from knowledge of that
// release; the package is not a dependency) for a batch of envs, as a loop of three launches per env step next to the (unchanged) step launch: the step, the
// episode ledger, the fused deterministic actor.  Included into the base translation unit only (hrgym_hip.hip, HRG_BASE_TU), after hrgym_ppo.h; it uses
// hrgym_buffer.h (the policy's view of a row, the episode tracker), hrgym_her.h's feature row and hrgym_mlp.h / hrgym_sac.h's tile products as they are.  No
// atomics, no waiting of one workgroup on another, every loop bound known at launch.
//
//   hrg_eval_begin_kernel      after a reset: the rows the episodes start from, the envs' quotas, the policy's view of the first rows.  One wavefront per env.
//   hrg_eval_step_kernel       after a step: Monitor's return and length, on a done step within the quota one record, then the policy's view of the next row.
//                              One wavefront per env, lane j writes column j of a record.
//   hrg_eval_remaining_kernel  sum over the envs of quota - count, one workgroup, a fixed order: what the host reads every few steps.
//   hrg_eval_policy_kernel     grid (ceil(m / MLP_T), P): tile (t, k) runs the deterministic actor of parameter set k on rows k m + 32 t .. of the view and writes
//                              the envs' action rows in double at the env's scale.
//
// The batch is P groups of m consecutive envs (n = P m), group k evaluated with parameter set k.  Within a group env e has the local index i = e % m and the quota
// (N + i) / m (integer division) of N episodes: SB3's episode_count_targets, which keeps a batch of envs from over-counting short episodes.  Once an env has met
// its quota its further steps leave the ledger untouched (the env goes on stepping: the batch is one launch).
//
// A record (HRG_EVAL_RECORD_DIM doubles): the return (Monitor's: the env's own reward, summed in double in step order), the length, the index of the finishing
// step since `begin`, TimeLimit.truncated, the HRG_INFO_DIM info columns of the last step, the episode's imitation reward sum.  Records are [n][max_quota][.],
// record c of env e its c-th finished episode; the host puts them into SB3's append order (finishing step, then env).
//
// The actions at the env's scale are the mappings of HipVecEnv.collect_steps / collect_rollout, rounded like torch's: SAC low + 0.5 (a + 1) (high - low) in
// double, every operation rounded on its own (no contraction into an FMA); PPO clamp(a, low, high) in float32.  Columns behind act_dim are zero.
#pragma once

// one hrg_eval: its sizes and switches (from hrg_eval_desc) and its buffers; passed to the kernels by value
struct EvalDev {
  EpisodeTracker ep;            // cur_obs, run_ret, run_len (acc is not kept: the ledger holds every episode)
  float* cur_time = nullptr;    // [n] the time value of the env's current row
  int32_t* count = nullptr;     // [n] records written
  int32_t* quota = nullptr;     // [n]
  double* records = nullptr;    // [n][max_quota][HRG_EVAL_RECORD_DIM]
  int64_t* remaining = nullptr; // [1]
  const double* act_low = nullptr;    // [HRG_ACT_DIM]
  const double* act_high = nullptr;   // [HRG_ACT_DIM]
  BufferView view;              // hrg_eval_desc: obs_cols, observe_time, mean / std, squash
  int32_t n_envs = 0, n_policies = 0, group = 0, n_episodes = 0, max_quota = 0, act_dim = 0, goal_env = 0, goal_kind = 0, width = 0;
};

// the actor of a learner, by the offsets of its handle (SacDev / PpoDev): hidden layers, the head's weights and biases, the head's outputs
struct EvalActor {
  int32_t w[HRG_SAC_MAX_DEPTH] = {0}, b[HRG_SAC_MAX_DEPTH] = {0}, hw = 0, hb = 0, nout = 0, depth = 0, K = 0, A = 0, n_params = 0;
};

// value `lane` of the policy's view of the row whose column `lane` is x (time value t): the flat view of hrgym_buffer.h, or the feature row of hrgym_her.h.
// Every lane of the wave takes part (the shuffles).
DI float eval_view(const EvalDev& h, float x, float t, int lane) {
  if (h.goal_env) {   // (uniform)
    const int ng = her_dg_dim(h.goal_kind);
    const float goal = __shfl(x, her_dg_col(h.goal_kind, lane < ng ? lane : 0));
    return her_feature(h.goal_kind, h.view.n_obs_cols, x, goal, view_select(h.view, x, lane), lane);
  }
  return replay_view(h.view, x, t, lane);
}

// grid = n_envs blocks of one wavefront; time may be null without observe_time
__global__ __launch_bounds__(64) void hrg_eval_begin_kernel(const EvalDev h, const float* __restrict__ obs, const float* __restrict__ time, float* __restrict__ view) {
  const int e = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (e >= h.n_envs) return;
  tracker_start(h.ep, e, lane, obs);
  const float t = h.view.observe_time ? time[e] : 0.0f;
  const float v = eval_view(h, obs[(size_t)e * HRG_OBS_DIM + lane], t, lane);
  if (lane < h.width) view[(size_t)e * h.width + lane] = v;
  if (lane == 0) {
    h.cur_time[e] = t;
    h.count[e] = 0;
    h.quota[e] = (h.n_episodes + e % h.group) / h.group;   // episode_count_targets within the group
  }
}

// grid = n_envs blocks of one wavefront; step: index of this step since begin.  imit / sir: the step's imitation rows or null (at most one of them; sir is there
// with observe_time -- the host checks both).
__global__ __launch_bounds__(64) void hrg_eval_step_kernel(const EvalDev h, int64_t step, const float* __restrict__ obs, const float* __restrict__ reward,
                                                           const uint8_t* __restrict__ done, const int32_t* __restrict__ info, const float* __restrict__ imit,
                                                           const float* __restrict__ sir, float* __restrict__ view) {
  const int e = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (e >= h.n_envs) return;
  const bool dn = done[e] != 0;
  const float* srow = sir ? sir + (size_t)e * HRG_SIR_DIM : nullptr;
  const float* irow = imit ? imit + (size_t)e * HRG_IMIT_DIM : nullptr;
  const int32_t* inf = info + (size_t)e * HRG_INFO_DIM;
  const float r = reward[e];
  const float r_env = srow ? srow[HRG_SIR_R_ENV] : irow ? irow[HRG_IMIT_R_ENV] : r;   // Monitor sits inside the imitation wrapper: its return is the env's own reward
  const double ep_im = !dn ? 0.0 : srow ? (double)srow[HRG_SIR_EP_IM] : irow ? (double)irow[HRG_IMIT_EP_IM] : 0.0;
  const double ep_ret = h.ep.run_ret[e] + (double)r_env;   // (the same value on every lane; read ahead of lane 0's write in tracker_step)
  const int32_t ep_len = h.ep.run_len[e] + 1;
  const int32_t c = h.count[e], q = h.quota[e];
  tracker_step(h.ep, e, lane, r_env, dn, inf, 0, 0.0);   // the running return and length; no sums over episodes
  if (dn && c < q && c < h.max_quota) {   // (uniform over the wave)
    if (lane < HRG_EVAL_RECORD_DIM) {
      const double x = lane == HRG_EVAL_REC_RETURN ? ep_ret : lane == HRG_EVAL_REC_LENGTH ? (double)ep_len : lane == HRG_EVAL_REC_STEP ? (double)step
                       : lane == HRG_EVAL_REC_TRUNCATED ? (inf[HRG_INFO_TRUNCATED] != 0 ? 1.0 : 0.0)
                       : lane < HRG_EVAL_REC_INFO + HRG_INFO_DIM ? (double)inf[lane - HRG_EVAL_REC_INFO] : ep_im;
      h.records[((size_t)e * (size_t)h.max_quota + (size_t)c) * HRG_EVAL_RECORD_DIM + lane] = x;
    }
    if (lane == 0) h.count[e] = c + 1;
  }
  // the policy's view of the next row: after an auto-reset the new episode's first row, with the time value the row carries
  const float o = obs[(size_t)e * HRG_OBS_DIM + lane];
  const float t_obs = h.view.observe_time ? srow[HRG_SIR_TIME_OBS] : 0.0f;
  const float v = eval_view(h, o, t_obs, lane);
  if (lane < h.width) view[(size_t)e * h.width + lane] = v;
  h.ep.cur_obs[(size_t)e * HRG_OBS_DIM + lane] = o;
  if (lane == 0) h.cur_time[e] = t_obs;
}

// one workgroup: thread t sums the envs t, t + 256, .. ascending, thread 0 the 256 partial sums ascending
__global__ __launch_bounds__(MLP_BLOCK) void hrg_eval_remaining_kernel(const EvalDev h) {
  __shared__ int64_t red[MLP_BLOCK];
  const int t = (int)threadIdx.x;
  int64_t mine = 0;
  for (int e = t; e < h.n_envs; e += MLP_BLOCK) mine += (int64_t)(h.quota[e] - h.count[e]);
  red[t] = mine;
  __syncthreads();
  if (t == 0) {
    int64_t sum = 0;
    for (int i = 0; i < MLP_BLOCK; i++) sum += red[i];
    h.remaining[0] = sum;
  }
}

// SB3's unscale_action in double as torch evaluates low + 0.5 * (a + 1.0) * (high - low): four operations, each rounded, none contracted into an FMA
DI double eval_unscale(double a, double low, double high) {
#pragma clang fp contract(off)
  const double half = 0.5 * (a + 1.0);
  const double span = high - low;
  const double scaled = half * span;
  return low + scaled;
}

// grid (ceil(m / MLP_T), P), MLP_BLOCK threads.  SAC: the actor a_w / a_b / a_hw / a_hb with ReLU units, tanh(mu) through sac_squash with zero noise, unscaled to
// the bounds.  PPO (SAC = false): the policy network with tanh units, mu, clamped to the bounds.  P: float [n_policies][n_params]; view: float [n][width];
// actions: double [n][HRG_ACT_DIM].  Rows behind the group's end are zero in the tile and are not stored.
template <bool SAC>
__global__ __launch_bounds__(MLP_BLOCK) void hrg_eval_policy_kernel(const EvalDev h, const EvalActor a, const float* __restrict__ P, const float* __restrict__ view,
                                                                    double* __restrict__ actions) {
  __shared__ MlpLds s;
  const int row0 = (int)blockIdx.x * MLP_T, k = (int)blockIdx.y, m = h.group, K = a.K, A = a.A;
  if (row0 >= m || k >= h.n_policies) return;   // (uniform over the workgroup)
  const float* Pk = P + (size_t)k * (size_t)a.n_params;
  const size_t env0 = (size_t)k * (size_t)m;
  mlp_load(s, view + env0 * (size_t)K, K, 0, row0, m);
  if (SAC)
    for (int i = (int)threadIdx.x; i < MLP_T * 8; i += (int)blockDim.x) s.eps[i] = 0.0f;
  mlp_trunk(s, Pk, a.w, a.b, a.depth, K, SAC ? MLP_ACT_RELU : MLP_ACT_TANH);
  mlp_head(s, Pk, a.hw, a.hb, a.depth, a.nout);
  if (SAC) {
    sac_squash(s, A);
    __syncthreads();
  }
  for (int i = (int)threadIdx.x; i < MLP_T * HRG_ACT_DIM; i += (int)blockDim.x) {
    const int r = i / HRG_ACT_DIM, j = i % HRG_ACT_DIM;
    if (row0 + r >= m) continue;
    double x = 0.0;
    if (j < A) {
      if (SAC) {
        x = eval_unscale((double)s.act[r * 8 + j], h.act_low[j], h.act_high[j]);
      } else {
        const float mu = (float)((double)s.D[r * MLP_DLD + j] + 0.0);   // hrg_ppo_forward_kernel's deterministic action: mu + exp(log_std) 0
        x = mu != mu ? (double)mu : (double)fminf(fmaxf(mu, (float)h.act_low[j]), (float)h.act_high[j]);   // torch.clamp hands a NaN on
      }
    }
    actions[(env0 + (size_t)(row0 + r)) * HRG_ACT_DIM + j] = x;
  }
}
