// hrgym_host_buffers.h -- the training buffers of the C ABI (include/hrgym.h): hindsight experience replay (hrg_her_*, hrg_goal_reward_done), the PPO rollout buffer
// (hrg_rollout_*) and the uniform replay buffer (hrg_replay_*), with what they check and upload alike.  Included by the base unit only, behind hrgym_host.h.

// What every buffer checks of its observation columns and action width, and the column table on the current device: obs_cols, zero behind n_obs_cols (a per-lane
// lookup).  `name`: the buffer's message prefix; observe_time: the descriptor's switch, null for a buffer without a time column.
static int buffer_columns(const char* name, int32_t n_obs_cols, const int32_t* obs_cols, const int32_t* observe_time, int32_t act_dim, DeviceMem& mem,
                          const int32_t*& table) {
  const std::string pre = std::string(name) + ": ";
  if (n_obs_cols < 1 || n_obs_cols + (observe_time && *observe_time ? 1 : 0) > HRG_OBS_DIM)
    return fail(HRG_ERR_INVALID, pre + (observe_time ? "n_obs_cols (+ 1 with observe_time) must lie in [1, HRG_OBS_DIM]" : "n_obs_cols must lie in [1, HRG_OBS_DIM]"));
  int32_t cols[HRG_OBS_DIM] = {0};
  for (int c = 0; c < n_obs_cols; c++) {
    if (obs_cols[c] < 0 || obs_cols[c] >= HRG_OBS_DIM) return fail(HRG_ERR_INVALID, pre + "an observation column outside the superset");
    cols[c] = obs_cols[c];
  }
  if (act_dim < 1 || act_dim > HRG_ACT_DIM) return fail(HRG_ERR_INVALID, pre + "act_dim must lie in [1, HRG_ACT_DIM]");
  return mem.upload(table, cols, HRG_OBS_DIM) ? HRG_OK : nomem(name, mem);
}

// What the replay buffer and the evaluator check of DatasetObsNormWrapper's statistics: mean / sd become the tables the view reads (mean 0 and std 1 behind the K
// values, and everywhere without normalize).  `name`: the message prefix.
static int view_statistics(const char* name, int K, int32_t normalize, int32_t squash, double squash_factor, const double* mean_in, const double* std_in, double* mean,
                           double* sd) {
  const std::string pre = std::string(name) + ": ";
  if (squash && !normalize) return fail(HRG_ERR_INVALID, pre + "squash needs normalize");
  for (int k = 0; k < HRG_OBS_DIM; k++) {
    mean[k] = normalize && k < K ? mean_in[k] : 0.0;
    sd[k] = normalize && k < K ? std_in[k] : 1.0;
    if (!std::isfinite(mean[k]) || !std::isfinite(sd[k]) || sd[k] == 0.0) return fail(HRG_ERR_INVALID, pre + "mean must be finite, std finite and non-zero");
  }
  if (normalize && squash && !std::isfinite(squash_factor)) return fail(HRG_ERR_INVALID, pre + "squash_factor must be finite");
  return HRG_OK;
}

// ... and the two tables on the current device, behind the view's pointers (synchronous)
static int view_statistics_upload(const char* name, DeviceMem& mem, BufferView& v, const double* mean, const double* sd) {
  if (!(mem.upload(v.mean, mean, HRG_OBS_DIM) && mem.upload(v.std, sd, HRG_OBS_DIM))) return nomem(name, mem);
  if (hipDeviceSynchronize() != hipSuccess) return fail(HRG_ERR_HIP, std::string(name) + ": upload failed");
  return HRG_OK;
}

extern "C" {

// ---- hindsight experience replay (csrc/hrgym_her.h) ----
struct hrg_her {
  int device = 0;
  hrg_her_desc desc;
  HerDev d;
  DeviceMem mem;                // behind every pointer of `d`
  int64_t* d_total = nullptr;   // pinned host word the sampler's total is read back into
  uint64_t calls = 0;           // sample calls so far (key of the draws)
  ~hrg_her() {
    if (d_total) hipHostFree(d_total);
  }
};

static int her_desc_check(const hrg_her_desc* p, bool ring) {
  if (p->goal_kind != HRG_GOAL_REACH && p->goal_kind != HRG_GOAL_CUBE) return fail(HRG_ERR_UNSUPPORTED, "her: unknown goal kind");
  if (!ring) return HRG_OK;
  if (p->strategy != HRG_HER_FUTURE && p->strategy != HRG_HER_FINAL && p->strategy != HRG_HER_EPISODE) return fail(HRG_ERR_UNSUPPORTED, "her: unknown goal selection strategy");
  if (p->n_envs < 1 || p->horizon < 1) return fail(HRG_ERR_INVALID, "her: n_envs and horizon must be positive");
  if (p->capacity <= p->horizon) return fail(HRG_ERR_INVALID, "her: capacity must exceed the horizon (a whole episode and one more transition have to fit the ring)");
  return HRG_OK;
}

// the rest of the descriptor, behind buffer_columns (n_obs_cols and act_dim are in range)
static int her_goal_check(const hrg_her_desc* p) {
  const int ng = p->goal_kind == HRG_GOAL_REACH ? 6 : 3;
  if (p->n_dg_in_obs != 0 && p->n_dg_in_obs != ng) return fail(HRG_ERR_INVALID, "her: n_dg_in_obs must be 0 or the goal's length");
  for (int d = 0; d < p->n_dg_in_obs; d++)
    if (p->dg_in_obs[d] < 0 || p->dg_in_obs[d] >= p->n_obs_cols) return fail(HRG_ERR_INVALID, "her: dg_in_obs outside the observation");
  if (!(p->her_ratio >= 0 && p->her_ratio <= 1)) return fail(HRG_ERR_INVALID, "her: her_ratio must lie in [0, 1]");
  if (p->rescale_actions)
    for (int k = 0; k < p->act_dim; k++)
      if (!(p->act_high[k] > p->act_low[k])) return fail(HRG_ERR_INVALID, "her: rescale_actions needs act_high > act_low");
  return HRG_OK;
}

int hrg_her_create(const hrg_her_desc* desc, int32_t device, hrg_her** out) {
  if (!desc || !out) return fail(HRG_ERR_INVALID, "null argument");
  *out = nullptr;
  int rc = her_desc_check(desc, true);
  if (rc != HRG_OK) return rc;
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<hrg_her> h(new hrg_her());
  h->device = device;
  h->desc = *desc;
  HerDev& d = h->d;
  DeviceMem& m = h->mem;
  rc = buffer_columns("her", desc->n_obs_cols, desc->obs_cols, nullptr, desc->act_dim, m, d.view.obs_cols);
  if (rc == HRG_OK) rc = her_goal_check(desc);
  if (rc != HRG_OK) return rc;
  d.view.n_obs_cols = desc->n_obs_cols;
  const size_t n = (size_t)desc->n_envs, slots = n * (size_t)desc->capacity;
  if (!(m.zeros(d.pre, slots * HRG_OBS_DIM) && m.zeros(d.post, slots * HRG_OBS_DIM) && m.zeros(d.act, slots * (size_t)desc->act_dim) && m.zeros(d.reward, slots) &&
        m.zeros(d.done, slots) && m.zeros(d.trunc, slots) && m.zeros(d.ctype, slots) && m.zeros(d.ep_start, slots) && m.zeros(d.ep_len, slots) && m.zeros(d.w, n) &&
        m.zeros(d.tail, n) && m.zeros(d.open, n) && m.zeros(d.ep.cur_obs, n * HRG_OBS_DIM) && m.zeros(d.ep.run_ret, n) && m.zeros(d.ep.run_len, n) &&
        m.zeros(d.ep.acc, n * HRG_HER_STATS_DIM)))
    return nomem("her", m);
  if (hipHostMalloc((void**)&h->d_total, sizeof(int64_t)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(HRG_ERR_HIP, "her: upload failed");
  *out = h.release();
  return HRG_OK;
}

void hrg_her_destroy(hrg_her* h) { destroy_handle(h); }

int hrg_her_observe(hrg_her* h, const float* obs_dev, const uint8_t* mask_dev, int64_t* counts_dev, void* stream) {
  if (!h || !obs_dev) return fail(HRG_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(h->device));
  return launch_per_env(hrg_her_observe_kernel, h->desc.n_envs, stream, h->desc, h->d, obs_dev, mask_dev, counts_dev);
}

int hrg_her_add(hrg_her* h, const double* actions_dev, const float* obs_dev, const float* term_obs_dev, const float* reward_dev, const uint8_t* done_dev,
                const int32_t* info_dev, int64_t* counts_dev, void* stream) {
  if (!h || !actions_dev || !obs_dev || !term_obs_dev || !reward_dev || !done_dev || !info_dev) return fail(HRG_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(h->device));
  return launch_per_env(hrg_her_add_kernel, h->desc.n_envs, stream, h->desc, h->d, actions_dev, obs_dev, term_obs_dev, reward_dev, done_dev, info_dev, counts_dev);
}

int hrg_her_sample(hrg_her* h, int32_t batch_size, const int64_t* counts_cum_dev, float* observation_dev, float* achieved_goal_dev, float* desired_goal_dev,
                   float* next_observation_dev, float* next_achieved_goal_dev, float* next_desired_goal_dev, float* action_dev, float* reward_dev,
                   float* done_dev, int64_t* index_dev, void* stream) {
  if (!h || !counts_cum_dev) return fail(HRG_ERR_INVALID, "null argument");
  if (batch_size < 1) return fail(HRG_ERR_INVALID, "her: batch_size must be positive");
  if (!observation_dev || !achieved_goal_dev || !desired_goal_dev || !next_observation_dev || !next_achieved_goal_dev || !next_desired_goal_dev || !action_dev ||
      !reward_dev || !done_dev)
    return fail(HRG_ERR_INVALID, "her: null output");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpyAsync(h->d_total, counts_cum_dev + h->desc.n_envs, sizeof(int64_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  if (*h->d_total < 1) return fail(HRG_ERR_INVALID, "her: no finished episode in the buffer yet (nothing to sample)");
  const int rc = launch_per_wave(hrg_her_sample_kernel, batch_size, stream, h->desc, h->d, counts_cum_dev, h->calls, (int)batch_size, observation_dev, achieved_goal_dev,
                                 desired_goal_dev, next_observation_dev, next_achieved_goal_dev, next_desired_goal_dev, action_dev, reward_dev, done_dev, index_dev);
  if (rc != HRG_OK) return rc;
  h->calls++;
  return HRG_OK;
}

// the width of the feature row achieved_goal | desired_goal | observation; the feature kernels keep one value per lane
static int her_feature_dim(const hrg_her_desc& p) { return (p.goal_kind == HRG_GOAL_REACH ? 6 + 6 : 7 + 3) + p.n_obs_cols; }
static int her_feature_check(const hrg_her_desc& p) {
  if (her_feature_dim(p) > HRG_OBS_DIM) return fail(HRG_ERR_INVALID, "her: achieved_goal + desired_goal + observation exceed HRG_OBS_DIM values (the feature kernels keep one per lane)");
  return HRG_OK;
}

int hrg_her_sample_features(hrg_her* h, int32_t batch_size, const int64_t* counts_cum_dev, float* features_dev, float* next_features_dev, float* action_dev,
                            float* reward_dev, float* done_dev, int64_t* index_dev, void* stream) {
  if (!h || !counts_cum_dev) return fail(HRG_ERR_INVALID, "null argument");
  if (batch_size < 1) return fail(HRG_ERR_INVALID, "her: batch_size must be positive");
  if (!features_dev || !next_features_dev || !action_dev || !reward_dev || !done_dev) return fail(HRG_ERR_INVALID, "her: null output");
  int rc = her_feature_check(h->desc);
  if (rc != HRG_OK) return rc;
  HIPCHK(hipSetDevice(h->device));
  rc = launch_per_wave(hrg_her_sample_features_kernel, batch_size, stream, h->desc, h->d, counts_cum_dev, h->calls, (int)batch_size, features_dev, next_features_dev,
                       action_dev, reward_dev, done_dev, index_dev);
  if (rc != HRG_OK) return rc;
  h->calls++;
  return HRG_OK;
}

int hrg_her_features(hrg_her* h, const float* rows_dev, int32_t n_rows, float* out_dev, void* stream) {
  if (!h || !out_dev) return fail(HRG_ERR_INVALID, "null argument");
  if (!rows_dev) {   // the envs' current rows
    rows_dev = h->d.ep.cur_obs;
    n_rows = h->desc.n_envs;
  }
  if (n_rows < 1) return fail(HRG_ERR_INVALID, "her: n_rows must be positive");
  const int rc = her_feature_check(h->desc);
  if (rc != HRG_OK) return rc;
  HIPCHK(hipSetDevice(h->device));
  return launch_per_wave(hrg_her_features_kernel, n_rows, stream, h->d.view, (int)h->desc.goal_kind, rows_dev, (int)n_rows, out_dev);
}

int hrg_her_stats(hrg_her* h, double* per_env_host, int32_t clear) {
  if (!h || !per_env_host) return fail(HRG_ERR_INVALID, "null argument");
  return buffer_stats(h->device, h->d.ep.acc, h->desc.n_envs, HRG_HER_STATS_DIM, per_env_host, clear);
}

int hrg_her_counts(hrg_her* h, int64_t* counts_host) {
  if (!h || !counts_host) return fail(HRG_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipDeviceSynchronize());
  const size_t n = (size_t)h->desc.n_envs;
  std::vector<int64_t> w(n), tail(n), open(n);
  HIPCHK(hipMemcpy(w.data(), h->d.w, sizeof(int64_t) * n, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(tail.data(), h->d.tail, sizeof(int64_t) * n, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(open.data(), h->d.open, sizeof(int64_t) * n, hipMemcpyDeviceToHost));
  counts_host[0] = counts_host[1] = 0;
  for (size_t e = 0; e < n; e++) { counts_host[0] += w[e] - tail[e]; counts_host[1] += open[e] - tail[e]; }
  counts_host[2] = (int64_t)h->calls;
  return HRG_OK;
}

int hrg_her_export(hrg_her* h, int32_t env, float* pre_host, float* post_host, float* action_host, float* reward_host, uint8_t* done_host,
                   uint8_t* truncated_host, int32_t* ctype_host, int64_t* ep_start_host, int32_t* ep_len_host, int64_t* state_host, float* cur_obs_host) {
  if (!h || !pre_host || !post_host || !action_host || !reward_host || !done_host || !truncated_host || !ctype_host || !ep_start_host || !ep_len_host || !state_host ||
      !cur_obs_host)
    return fail(HRG_ERR_INVALID, "null argument");
  if (env < 0 || env >= h->desc.n_envs) return fail(HRG_ERR_INVALID, "bad env index");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipDeviceSynchronize());
  const HerDev& d = h->d;
  const size_t cap = (size_t)h->desc.capacity, r0 = (size_t)env * cap, row = sizeof(float) * HRG_OBS_DIM, ad = (size_t)h->desc.act_dim;
  HIPCHK(hipMemcpy(pre_host, d.pre + r0 * HRG_OBS_DIM, cap * row, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(post_host, d.post + r0 * HRG_OBS_DIM, cap * row, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(action_host, d.act + r0 * ad, cap * ad * sizeof(float), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(reward_host, d.reward + r0, cap * sizeof(float), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(done_host, d.done + r0, cap, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(truncated_host, d.trunc + r0, cap, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(ctype_host, d.ctype + r0, cap * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(ep_start_host, d.ep_start + r0, cap * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(ep_len_host, d.ep_len + r0, cap * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(state_host + 0, d.w + env, sizeof(int64_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(state_host + 1, d.tail + env, sizeof(int64_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(state_host + 2, d.open + env, sizeof(int64_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(cur_obs_host, d.ep.cur_obs + (size_t)env * HRG_OBS_DIM, row, hipMemcpyDeviceToHost));
  return HRG_OK;
}

int hrg_goal_reward_done(const hrg_her_desc* desc, const float* ag_dev, const float* dg_dev, const int32_t* ctype_dev, int32_t n, float* reward_dev,
                         uint8_t* done_dev, void* stream) {
  if (!desc || !ag_dev || !dg_dev || !ctype_dev || !reward_dev || !done_dev) return fail(HRG_ERR_INVALID, "null argument");
  if (n < 1) return fail(HRG_ERR_INVALID, "her: n must be positive");
  const int rc = her_desc_check(desc, false);
  if (rc != HRG_OK) return rc;
  hipLaunchKernelGGL(hrg_goal_reward_done_kernel, dim3(((unsigned)n + HRG_BUFFER_BLOCK - 1) / HRG_BUFFER_BLOCK), dim3(HRG_BUFFER_BLOCK), 0, (hipStream_t)stream, *desc, ag_dev, dg_dev,
                     ctype_dev, (int)n, reward_dev, done_dev);
  HIPCHK(hipGetLastError());
  return HRG_OK;
}

// ---- PPO rollout buffer (csrc/hrgym_rollout.h) ----
struct hrg_rollout {
  int device = 0;
  hrg_rollout_desc desc;
  RolloutDev d;
  DeviceMem mem;           // behind every pointer of `d`
  int32_t pos = 0;         // the next slot (the write position lives on the host)
  bool computed = false;   // advantages and returns belong to the stored steps
};

int hrg_rollout_create(const hrg_rollout_desc* desc, int32_t device, hrg_rollout** out) {
  if (!desc || !out) return fail(HRG_ERR_INVALID, "null argument");
  *out = nullptr;
  if (desc->n_envs < 1 || desc->n_steps < 1) return fail(HRG_ERR_INVALID, "rollout: n_envs and n_steps must be positive");
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<hrg_rollout> h(new hrg_rollout());
  h->device = device;
  h->desc = *desc;
  RolloutDev& d = h->d;
  DeviceMem& m = h->mem;
  const int rc = buffer_columns("rollout", desc->n_obs_cols, desc->obs_cols, nullptr, desc->act_dim, m, d.view.obs_cols);
  if (rc != HRG_OK) return rc;
  if (!(desc->gamma >= 0 && desc->gamma <= 1)) return fail(HRG_ERR_INVALID, "rollout: gamma must lie in [0, 1]");
  if (!(desc->gae_lambda >= 0 && desc->gae_lambda <= 1)) return fail(HRG_ERR_INVALID, "rollout: gae_lambda must lie in [0, 1]");
  d.view.n_obs_cols = desc->n_obs_cols;
  const size_t n = (size_t)desc->n_envs, slots = n * (size_t)desc->n_steps;
  if (!(m.zeros(d.obs, slots * (size_t)desc->n_obs_cols) && m.zeros(d.act, slots * (size_t)desc->act_dim) && m.zeros(d.reward, slots) && m.zeros(d.value, slots) &&
        m.zeros(d.log_prob, slots) && m.zeros(d.ep_start, slots) && m.zeros(d.adv, slots) && m.zeros(d.ret, slots) && m.zeros(d.flag, n) &&
        m.zeros(d.ep.cur_obs, n * HRG_OBS_DIM) && m.zeros(d.ep.run_ret, n) && m.zeros(d.ep.run_len, n) && m.zeros(d.ep.acc, n * HRG_ROLLOUT_STATS_DIM)))
    return nomem("rollout", m);
  if (hipDeviceSynchronize() != hipSuccess) return fail(HRG_ERR_HIP, "rollout: upload failed");
  *out = h.release();
  return HRG_OK;
}

void hrg_rollout_destroy(hrg_rollout* h) { destroy_handle(h); }

int hrg_rollout_view(hrg_rollout* h, const float* rows_dev, int32_t n_rows, float* out_dev, void* stream) {
  if (!h || !out_dev) return fail(HRG_ERR_INVALID, "null argument");
  if (!rows_dev) {   // the envs' current rows
    rows_dev = h->d.ep.cur_obs;
    n_rows = h->desc.n_envs;
  }
  if (n_rows < 1) return fail(HRG_ERR_INVALID, "rollout: n_rows must be positive");
  HIPCHK(hipSetDevice(h->device));
  return launch_per_wave(hrg_buffer_view_kernel, n_rows, stream, h->d.view, rows_dev, (const float*)nullptr, (int)n_rows, out_dev);
}

int hrg_rollout_observe(hrg_rollout* h, const float* obs_dev, const uint8_t* mask_dev, void* stream) {
  if (!h || !obs_dev) return fail(HRG_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(h->device));
  return launch_per_env(hrg_rollout_observe_kernel, h->desc.n_envs, stream, h->desc, h->d, obs_dev, mask_dev);
}

int hrg_rollout_add(hrg_rollout* h, const float* actions_dev, const float* values_dev, const float* log_probs_dev, const float* terminal_values_dev,
                    const float* obs_dev, const float* reward_dev, const uint8_t* done_dev, const int32_t* info_dev, void* stream) {
  if (!h || !actions_dev || !values_dev || !log_probs_dev || !obs_dev || !reward_dev || !done_dev || !info_dev) return fail(HRG_ERR_INVALID, "null argument");
  if (h->pos >= h->desc.n_steps) return fail(HRG_ERR_INVALID, "rollout: the buffer is full (hrg_rollout_reset starts the next rollout)");
  HIPCHK(hipSetDevice(h->device));
  const int rc = launch_per_env(hrg_rollout_add_kernel, h->desc.n_envs, stream, h->desc, h->d, (int)h->pos, actions_dev, values_dev, log_probs_dev, terminal_values_dev, obs_dev,
                                reward_dev, done_dev, info_dev);
  if (rc != HRG_OK) return rc;
  h->pos++;
  h->computed = false;
  return HRG_OK;
}

int hrg_rollout_compute(hrg_rollout* h, const float* last_values_dev, void* stream) {
  if (!h || !last_values_dev) return fail(HRG_ERR_INVALID, "null argument");
  if (h->pos < h->desc.n_steps) return fail(HRG_ERR_INVALID, "rollout: the buffer is not full yet (returns and advantages are computed over n_steps steps)");
  HIPCHK(hipSetDevice(h->device));
  hipLaunchKernelGGL(hrg_rollout_gae_kernel, dim3(((unsigned)h->desc.n_envs + HRG_BUFFER_BLOCK - 1) / HRG_BUFFER_BLOCK), dim3(HRG_BUFFER_BLOCK), 0, (hipStream_t)stream, h->desc,
                     h->d, last_values_dev);
  HIPCHK(hipGetLastError());
  h->computed = true;
  return HRG_OK;
}

int hrg_rollout_get(hrg_rollout* h, const int64_t* index_dev, int32_t batch_size, float* observations_dev, float* actions_dev, float* old_values_dev,
                    float* old_log_prob_dev, float* advantages_dev, float* returns_dev, void* stream) {
  if (!h || !index_dev || !observations_dev || !actions_dev || !old_values_dev || !old_log_prob_dev || !advantages_dev || !returns_dev)
    return fail(HRG_ERR_INVALID, "null argument");
  if (batch_size < 1) return fail(HRG_ERR_INVALID, "rollout: batch_size must be positive");
  if (!h->computed) return fail(HRG_ERR_INVALID, "rollout: no returns and advantages yet (hrg_rollout_compute comes first)");
  HIPCHK(hipSetDevice(h->device));
  return launch_per_wave(hrg_rollout_get_kernel, batch_size, stream, h->desc, h->d, index_dev, (int)batch_size, observations_dev, actions_dev, old_values_dev, old_log_prob_dev,
                         advantages_dev, returns_dev);
}

int hrg_rollout_reset(hrg_rollout* h) {
  if (!h) return fail(HRG_ERR_INVALID, "null argument");
  h->pos = 0;
  h->computed = false;
  return HRG_OK;
}

int hrg_rollout_stats(hrg_rollout* h, double* per_env_host, int32_t clear) {
  if (!h || !per_env_host) return fail(HRG_ERR_INVALID, "null argument");
  return buffer_stats(h->device, h->d.ep.acc, h->desc.n_envs, HRG_ROLLOUT_STATS_DIM, per_env_host, clear);
}

int hrg_rollout_export(hrg_rollout* h, float* observations_host, float* actions_host, float* rewards_host, float* values_host, float* log_probs_host,
                       float* episode_starts_host, float* advantages_host, float* returns_host, float* cur_obs_host, float* flags_host, double* run_return_host,
                       int32_t* run_length_host, double* stats_host, int64_t* state_host) {
  if (!h || !observations_host || !actions_host || !rewards_host || !values_host || !log_probs_host || !episode_starts_host || !advantages_host || !returns_host ||
      !cur_obs_host || !flags_host || !run_return_host || !run_length_host || !stats_host || !state_host)
    return fail(HRG_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipDeviceSynchronize());
  const RolloutDev& d = h->d;
  const size_t n = (size_t)h->desc.n_envs, T = (size_t)h->desc.n_steps, slots = n * T;
  HIPCHK(hipMemcpy(observations_host, d.obs, slots * sizeof(float) * (size_t)h->desc.n_obs_cols, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(actions_host, d.act, slots * sizeof(float) * (size_t)h->desc.act_dim, hipMemcpyDeviceToHost));
  std::vector<float> tm(slots);   // a time-major array on its way into the flat order
  const float* scalars[6] = {d.reward, d.value, d.log_prob, d.ep_start, d.adv, d.ret};
  float* flat[6] = {rewards_host, values_host, log_probs_host, episode_starts_host, advantages_host, returns_host};
  for (int a = 0; a < 6; a++) {
    HIPCHK(hipMemcpy(tm.data(), scalars[a], slots * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t e = 0; e < n; e++)
      for (size_t t = 0; t < T; t++) flat[a][e * T + t] = tm[t * n + e];
  }
  HIPCHK(hipMemcpy(cur_obs_host, d.ep.cur_obs, n * sizeof(float) * HRG_OBS_DIM, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(flags_host, d.flag, n * sizeof(float), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(run_return_host, d.ep.run_ret, n * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(run_length_host, d.ep.run_len, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(stats_host, d.ep.acc, n * sizeof(double) * HRG_ROLLOUT_STATS_DIM, hipMemcpyDeviceToHost));
  state_host[0] = h->pos;
  state_host[1] = h->computed ? 1 : 0;
  return HRG_OK;
}

// ---- uniform replay buffer (csrc/hrgym_replay.h) ----
struct hrg_replay {
  int device = 0;
  hrg_replay_desc desc;
  ReplayDev d;
  int32_t pos = 0;      // the next slot (the write position lives on the host)
  bool full = false;    // every slot holds a transition
  uint64_t calls = 0;   // sample calls that drew their indices (key of the draws)
  uint64_t group_calls = 0;   // ... of the grouped sample (hrg_sac_population_sample), a counter of its own
  DeviceMem mem;        // behind every pointer of `d`
};

int hrg_replay_create(const hrg_replay_desc* desc, int32_t device, hrg_replay** out) {
  if (!desc || !out) return fail(HRG_ERR_INVALID, "null argument");
  *out = nullptr;
  if (desc->n_envs < 1 || desc->capacity < 1) return fail(HRG_ERR_INVALID, "replay: n_envs and capacity must be positive");
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<hrg_replay> h(new hrg_replay());
  h->device = device;
  h->desc = *desc;
  ReplayDev& d = h->d;
  BufferView& v = d.view;
  DeviceMem& m = h->mem;
  const size_t n = (size_t)desc->n_envs, slots = n * (size_t)desc->capacity;
  v.observe_time = desc->observe_time ? 1 : 0;
  const int K = desc->n_obs_cols + v.observe_time;
  const int rc = buffer_columns("replay", desc->n_obs_cols, desc->obs_cols, &desc->observe_time, desc->act_dim, m, v.obs_cols);
  if (rc != HRG_OK) return rc;
  double mean[HRG_OBS_DIM], sd[HRG_OBS_DIM];
  if (int rs = view_statistics("replay", K, desc->normalize, desc->squash, desc->squash_factor, desc->mean, desc->std, mean, sd)) return rs;
  d.n_envs = desc->n_envs; d.capacity = desc->capacity; d.act_dim = desc->act_dim; d.seed = desc->seed;
  v.n_obs_cols = desc->n_obs_cols; v.normalize = desc->normalize ? 1 : 0; v.squash = desc->squash ? 1 : 0; v.squash_factor = desc->squash_factor;
  if (!(m.zeros(d.obs, slots * (size_t)K) && m.zeros(d.nobs, slots * (size_t)K) && m.zeros(d.act, slots * (size_t)desc->act_dim) && m.zeros(d.reward, slots) &&
        m.zeros(d.done, slots) && m.zeros(d.timeout, slots) && m.zeros(d.cur_time, n) && m.zeros(d.ep.cur_obs, n * HRG_OBS_DIM) && m.zeros(d.ep.run_ret, n) &&
        m.zeros(d.ep.run_len, n) && m.zeros(d.ep.acc, n * HRG_REPLAY_STATS_DIM)))
    return nomem("replay", m);
  if (int ru = view_statistics_upload("replay", m, v, mean, sd)) return ru;
  *out = h.release();
  return HRG_OK;
}

void hrg_replay_destroy(hrg_replay* h) { destroy_handle(h); }

int hrg_replay_view(hrg_replay* h, const float* rows_dev, const float* time_dev, int32_t n_rows, float* out_dev, void* stream) {
  if (!h || !out_dev) return fail(HRG_ERR_INVALID, "null argument");
  if (!rows_dev) {   // the envs' current rows
    rows_dev = h->d.ep.cur_obs;
    time_dev = h->d.cur_time;
    n_rows = h->desc.n_envs;
  }
  if (n_rows < 1) return fail(HRG_ERR_INVALID, "replay: n_rows must be positive");
  if (h->d.view.observe_time && !time_dev) return fail(HRG_ERR_INVALID, "replay: observe_time needs the rows' time values");
  HIPCHK(hipSetDevice(h->device));
  return launch_per_wave(hrg_buffer_view_kernel, n_rows, stream, h->d.view, rows_dev, time_dev, (int)n_rows, out_dev);
}

int hrg_replay_observe(hrg_replay* h, const float* obs_dev, const float* time_dev, const uint8_t* mask_dev, void* stream) {
  if (!h || !obs_dev) return fail(HRG_ERR_INVALID, "null argument");
  if (h->d.view.observe_time && !time_dev) return fail(HRG_ERR_INVALID, "replay: observe_time needs the rows' time values");
  HIPCHK(hipSetDevice(h->device));
  return launch_per_env(hrg_replay_observe_kernel, h->desc.n_envs, stream, h->d, obs_dev, time_dev, mask_dev);
}

int hrg_replay_add(hrg_replay* h, const float* actions_dev, const float* obs_dev, const float* term_obs_dev, const float* reward_dev, const uint8_t* done_dev,
                   const int32_t* info_dev, const float* imit_dev, const float* sir_dev, void* stream) {
  if (!h || !actions_dev || !obs_dev || !term_obs_dev || !reward_dev || !done_dev || !info_dev) return fail(HRG_ERR_INVALID, "null argument");
  if (imit_dev && sir_dev) return fail(HRG_ERR_INVALID, "replay: an imitation row or a state imitation row, not both");
  if (h->d.view.observe_time && !sir_dev) return fail(HRG_ERR_INVALID, "replay: observe_time needs the state imitation rows (their time columns)");
  HIPCHK(hipSetDevice(h->device));
  const int rc = launch_per_env(hrg_replay_add_kernel, h->desc.n_envs, stream, h->d, (int)h->pos, actions_dev, obs_dev, term_obs_dev, reward_dev, done_dev, info_dev, imit_dev, sir_dev);
  if (rc != HRG_OK) return rc;
  if (++h->pos == h->desc.capacity) {   // ReplayBuffer.add: self.full = True; self.pos = 0
    h->pos = 0;
    h->full = true;
  }
  return HRG_OK;
}

// what both sample entries end with; seeds_dev null: one group under the buffer's seed
static int replay_sample(hrg_replay* h, int32_t n_groups, int32_t batch_size, const uint64_t* seeds_dev, uint64_t& calls, const int64_t* index_in_dev, float* observations_dev,
                         float* actions_dev, float* next_observations_dev, float* dones_dev, float* rewards_dev, int64_t* index_out_dev, void* stream) {
  if (batch_size < 1) return fail(HRG_ERR_INVALID, "replay: batch_size must be positive");
  if (!observations_dev || !actions_dev || !next_observations_dev || !dones_dev || !rewards_dev) return fail(HRG_ERR_INVALID, "replay: null output");
  const int64_t upper = h->full ? h->desc.capacity : h->pos;
  if (upper < 1) return fail(HRG_ERR_INVALID, "replay: the buffer is empty (nothing to sample)");
  HIPCHK(hipSetDevice(h->device));
  const int rc = launch_per_wave(hrg_replay_sample_kernel, n_groups * batch_size, stream, h->d, upper, calls, index_in_dev, (int)batch_size, (int)n_groups, seeds_dev,
                                 observations_dev, actions_dev, next_observations_dev, dones_dev, rewards_dev, index_out_dev);
  if (rc != HRG_OK) return rc;
  if (!index_in_dev) calls++;
  return HRG_OK;
}

int hrg_replay_sample(hrg_replay* h, int32_t batch_size, const int64_t* index_in_dev, float* observations_dev, float* actions_dev, float* next_observations_dev,
                      float* dones_dev, float* rewards_dev, int64_t* index_out_dev, void* stream) {
  if (!h) return fail(HRG_ERR_INVALID, "null argument");
  return replay_sample(h, 1, batch_size, nullptr, h->calls, index_in_dev, observations_dev, actions_dev, next_observations_dev, dones_dev, rewards_dev, index_out_dev, stream);
}

int hrg_sac_population_sample(hrg_replay* h, int32_t n_groups, int32_t batch_size, const uint64_t* seeds_dev, float* observations_dev, float* actions_dev,
                              float* next_observations_dev, float* dones_dev, float* rewards_dev, int64_t* index_out_dev, void* stream) {
  if (!h) return fail(HRG_ERR_INVALID, "null argument");
  if (n_groups < 1 || h->desc.n_envs % n_groups)
    return fail(HRG_ERR_INVALID, "replay: n_envs = " + std::to_string(h->desc.n_envs) + " is not divisible by n_groups = " + std::to_string(n_groups) +
                                     ": every member samples a group of the same size");
  if (!seeds_dev) return fail(HRG_ERR_INVALID, "replay: a grouped sample needs its seeds table (n_groups values on the device)");
  if ((int64_t)n_groups * batch_size > INT32_MAX) return fail(HRG_ERR_INVALID, "replay: n_groups * batch_size above the 2^31 - 1 rows of a launch");
  return replay_sample(h, n_groups, batch_size, seeds_dev, h->group_calls, nullptr, observations_dev, actions_dev, next_observations_dev, dones_dev, rewards_dev,
                       index_out_dev, stream);
}

int hrg_replay_stats(hrg_replay* h, double* per_env_host, int32_t clear) {
  if (!h || !per_env_host) return fail(HRG_ERR_INVALID, "null argument");
  return buffer_stats(h->device, h->d.ep.acc, h->desc.n_envs, HRG_REPLAY_STATS_DIM, per_env_host, clear);
}

int hrg_replay_export(hrg_replay* h, float* observations_host, float* next_observations_host, float* actions_host, float* rewards_host, uint8_t* dones_host,
                      uint8_t* timeouts_host, float* cur_obs_host, float* cur_time_host, double* run_return_host, int32_t* run_length_host, double* stats_host,
                      int64_t* state_host) {
  if (!h || !observations_host || !next_observations_host || !actions_host || !rewards_host || !dones_host || !timeouts_host || !cur_obs_host || !cur_time_host ||
      !run_return_host || !run_length_host || !stats_host || !state_host)
    return fail(HRG_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipDeviceSynchronize());
  const ReplayDev& d = h->d;
  const size_t n = (size_t)h->desc.n_envs, slots = n * (size_t)h->desc.capacity, K = (size_t)(d.view.n_obs_cols + d.view.observe_time);
  HIPCHK(hipMemcpy(observations_host, d.obs, slots * sizeof(float) * K, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(next_observations_host, d.nobs, slots * sizeof(float) * K, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(actions_host, d.act, slots * sizeof(float) * (size_t)d.act_dim, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(rewards_host, d.reward, slots * sizeof(float), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(dones_host, d.done, slots, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(timeouts_host, d.timeout, slots, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(cur_obs_host, d.ep.cur_obs, n * sizeof(float) * HRG_OBS_DIM, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(cur_time_host, d.cur_time, n * sizeof(float), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(run_return_host, d.ep.run_ret, n * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(run_length_host, d.ep.run_len, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(stats_host, d.ep.acc, n * sizeof(double) * HRG_REPLAY_STATS_DIM, hipMemcpyDeviceToHost));
  state_host[0] = h->pos;
  state_host[1] = h->full ? 1 : 0;
  state_host[2] = (int64_t)h->calls;
  return HRG_OK;
}

int hrg_replay_size(hrg_replay* h, int64_t* size_host) {
  if (!h || !size_host) return fail(HRG_ERR_INVALID, "null argument");
  size_host[0] = h->pos;
  size_host[1] = h->full ? 1 : 0;
  size_host[2] = (int64_t)h->calls;
  size_host[3] = (int64_t)h->mem.bytes;
  return HRG_OK;
}

} // extern "C"
