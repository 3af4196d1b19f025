// hrgym_her.h -- hindsight experience replay on the device: the replay buffer of SAC + HER (SB3's HerReplayBuffer with the reference's patches,
// wrappers/HER_buffer_add_monkey_patch.py) for a batch of goal envs, in six small kernels next to the (unchanged) step launch.  Included into the base
// translation unit only (hrgym_hip.hip, HRG_BASE_TU), after hrgym_buffer.h (the policy's view of a row, the episode tracker, the grid of the
// one-wavefront-per-sample kernels).
//
//   hrg_her_add_kernel           custom_add (26-117) for every env: one transition into the env's ring, episode bookkeeping.  One wavefront per env, lane l
//                                moves column l of each 256-byte observation row.
//   hrg_her_observe_kernel       the first observation of an episode after a reset; the unfinished episode of a reset env is discarded.
//   hrg_her_sample_kernel        _custom_sample_transitions (120-286), online sampling: one wavefront per sample, four per block, no LDS, no atomics.
//   hrg_her_sample_features_kernel  the same samples (her_draw: the draws, the relabelling, reward and done, the rewritten observation) as the rows a
//                                MultiInputPolicy's CombinedExtractor feeds its MLPs: features[k][F] and next_features[k][F], F = ag_dim + dg_dim + n_obs_cols
//                                <= 64, laid out achieved_goal | desired_goal | observation (gym.spaces.Dict orders its keys alphabetically).  Lane l < F stores
//                                value l: one coalesced row store per row.  Where the prefix sums' total is <= 0 the kernel returns and leaves its outputs
//                                unwritten (the caller checks for an empty buffer once per train call, not per sample).
//   hrg_her_features_kernel      the same feature row of caller-supplied rows of the superset, or of the envs' current rows (SB3's _last_obs): one wavefront
//                                per row, like hrg_buffer_view_kernel.
//   hrg_goal_reward_done_kernel  HumanEnv._compute_reward / _check_done of caller-supplied goal rows, one thread per row; the sample kernels call the same
//                                device function for their relabelled samples.
//
// Episode statistics: the shared tracker (hrgym_buffer.h) with HRG_HER_STATS_DIM columns; the return is the env's own step reward.  A masked observe starts the
// env's running return and length again, as it discards the env's open episode.
//
// The ring of env e: slot = write counter % capacity.  Three counters per env: w (next write), tail (oldest valid transition), open (first transition of
// the running episode); tail <= open <= w, w - tail <= capacity.  Every slot carries ep_start (counter of its episode's first transition) and ep_len (0 while
// the episode runs; back-filled over the episode when it ends).  When the ring is full the oldest episode leaves whole, so the closed transitions of an env
// are always the contiguous counter range [tail, open): the sampler needs one prefix sum over the envs and no episode table.
//
// Draws: rng_u01 keyed by (buffer seed, sample call counter, index of the sample in its batch, STREAM_HER, 0..2): independent of the grid and of the batch
// size, and no stream of the step / reset / expert / dataset kernels moves.
#pragma once

enum { STREAM_HER = 10 };   // after STREAM_DATASET = 9 (hrgym_dataset.h)
#define HRG_HER_STATS_DIM (3 + HRG_INFO_DIM)   // episodes, return, length, the info columns

// the buffers of one hrg_her; passed to the kernels by value
struct HerDev {
  float* pre = nullptr;        // [n][cap][HRG_OBS_DIM] the row before the step
  float* post = nullptr;       // [n][cap][HRG_OBS_DIM] the row after it (the terminal observation where the step finished the env)
  float* act = nullptr;        // [n][cap][act_dim]
  float* reward = nullptr;     // [n][cap]
  uint8_t* done = nullptr;     // [n][cap]
  uint8_t* trunc = nullptr;    // [n][cap] TimeLimit.truncated
  int32_t* ctype = nullptr;    // [n][cap] collision_type
  int64_t* ep_start = nullptr; // [n][cap]
  int32_t* ep_len = nullptr;   // [n][cap]
  int64_t* w = nullptr;        // [n]
  int64_t* tail = nullptr;     // [n]
  int64_t* open = nullptr;     // [n]
  EpisodeTracker ep;           // the current rows (the row the next transition starts from); the returns are the env's own reward; HRG_HER_STATS_DIM columns
  BufferView view;             // hrg_her_desc::obs_cols (the view is a plain selection: no time column, no normalisation)
};

// columns of the observation superset behind the goals (vec_env.HipVecEnv._init_columns)
DI int her_ag_dim(int kind) { return kind == HRG_GOAL_REACH ? 6 : 7; }
DI int her_dg_dim(int kind) { return kind == HRG_GOAL_REACH ? 6 : 3; }
DI int her_ag_col(int kind, int d) { return kind == HRG_GOAL_REACH ? 18 + d : d < 3 ? 30 + d : d < 6 ? 44 + d : 39; }   // joint positions | eef_pos, object_pos, object_gripped
DI int her_dg_col(int kind, int d) { return kind == HRG_GOAL_REACH ? 33 + d : 50 + d; }                               // desired_goal | target_pos
DI int her_new_goal_col(int kind, int d) { return kind == HRG_GOAL_REACH ? 18 + d : 47 + d; }                         // what a reached state offers as a goal

// HumanEnv._compute_reward (human_env.py:629-664, 766-792) and _check_done (835-858) of one goal pair, the arithmetic of HipVecEnv.compute_reward /
// compute_done: FP64 over the f32 values.  ag: her_ag_dim values, dg: her_dg_dim values.
DI void goal_reward_done(const hrg_her_desc& p, const double* ag, const double* dg, int ctype, float* reward, bool* done) {
  double r, dense, dist;
  if (p.goal_kind == HRG_GOAL_REACH) {
    double d2 = 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) { const double d = ag[k] - dg[k]; d2 += d * d; }
    dist = sqrt(d2);
    r = dist <= p.goal_dist ? p.task_reward : -1.0;
    dense = -0.1 * dist;
  } else {
    double a2 = 0.0, b2 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) { const double a = ag[3 + k] - ag[k], b = dg[k] - ag[3 + k]; a2 += a * a; b2 += b * b; }
    const double e2o = sqrt(a2);
    dist = sqrt(b2);
    r = dist <= p.goal_dist ? p.task_reward : ag[6] != 0.0 ? p.object_gripped_reward : -1.0;
    dense = -(e2o * 0.2 + dist) * 0.1;
  }
  if (p.reward_shaping) r = r + 1.0 + dense;
  const bool illegal = (ctype & (HRG_COL_STATIC | HRG_COL_ROBOT | HRG_COL_HUMAN_CRIT)) != 0;
  *reward = (float)((r + (illegal ? p.collision_reward : 0.0)) * p.reward_scale);
  *done = (p.done_at_collision != 0 && illegal) || (p.done_at_success != 0 && dist <= p.goal_dist);
}

__global__ __launch_bounds__(HRG_BUFFER_BLOCK) void hrg_goal_reward_done_kernel(const hrg_her_desc p, const float* __restrict__ ag, const float* __restrict__ dg,
                                                                             const int32_t* __restrict__ ctype, int n, float* __restrict__ reward,
                                                                             uint8_t* __restrict__ done) {
  const int i = (int)(blockIdx.x * HRG_BUFFER_BLOCK + threadIdx.x);
  if (i >= n) return;
  const int na = her_ag_dim(p.goal_kind), ng = her_dg_dim(p.goal_kind);
  double a[7], g[6];
#pragma unroll
  for (int k = 0; k < 7; k++) a[k] = k < na ? (double)ag[(size_t)i * na + k] : 0.0;
#pragma unroll
  for (int k = 0; k < 6; k++) g[k] = k < ng ? (double)dg[(size_t)i * ng + k] : 0.0;
  float r;
  bool d;
  goal_reward_done(p, a, g, ctype[i], &r, &d);
  reward[i] = r;
  done[i] = d ? 1 : 0;
}

// grid = n_envs blocks of one wavefront
__global__ __launch_bounds__(64) void hrg_her_add_kernel(const hrg_her_desc p, const HerDev h, const double* __restrict__ actions, const float* __restrict__ obs,
                                                         const float* __restrict__ term_obs, const float* __restrict__ reward, const uint8_t* __restrict__ done,
                                                         const int32_t* __restrict__ info, int64_t* __restrict__ counts) {
  const int e = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (e >= p.n_envs) return;
  const int64_t cap = p.capacity;
  int64_t w = h.w[e], tail = h.tail[e], open = h.open[e];
  const size_t ring = (size_t)e * (size_t)cap;
  if (w - tail == cap) {   // full: the oldest episode leaves whole
    const size_t ts = ring + (size_t)(tail % cap);
    const int32_t len = h.ep_len[ts];
    if (len > 0) tail = h.ep_start[ts] + len;
    else tail = open = w;   // an episode longer than the ring (the caller's horizon was wrong): it is dropped, the ring stays consistent
  }
  const size_t s = ring + (size_t)(w % cap);
  const bool dn = done[e] != 0;
  h.pre[s * HRG_OBS_DIM + lane] = h.ep.cur_obs[(size_t)e * HRG_OBS_DIM + lane];
  const float o = obs[(size_t)e * HRG_OBS_DIM + lane];
  h.post[s * HRG_OBS_DIM + lane] = dn ? term_obs[(size_t)e * HRG_OBS_DIM + lane] : o;
  h.ep.cur_obs[(size_t)e * HRG_OBS_DIM + lane] = o;   // after an auto-reset: the new episode's first row
  tracker_step(h.ep, e, lane, reward[e], dn, info + (size_t)e * HRG_INFO_DIM, HRG_HER_STATS_DIM, 0.0);
  if (lane < p.act_dim) {
    double a = actions[(size_t)e * HRG_ACT_DIM + lane];
    if (p.rescale_actions) {   // HER_buffer_add_monkey_patch.py:64-76
      a = 2.0 * ((a - p.act_low[lane]) / (p.act_high[lane] - p.act_low[lane])) - 1.0;
      a = fmin(fmax(a, -1.0), 1.0);
    }
    h.act[s * (size_t)p.act_dim + lane] = (float)a;
  }
  if (lane == 0) {
    h.reward[s] = reward[e];
    h.done[s] = dn ? 1 : 0;
    h.trunc[s] = info[(size_t)e * HRG_INFO_DIM + HRG_INFO_TRUNCATED] != 0 ? 1 : 0;
    h.ctype[s] = info[(size_t)e * HRG_INFO_DIM + HRG_INFO_COLLISION_TYPE];
    h.ep_start[s] = open;
    if (!dn) h.ep_len[s] = 0;   // (where done, the back-fill below writes it)
  }
  w++;
  if (dn) {
    const int64_t len = w - open;   // <= cap
    for (int64_t k = lane; k < len; k += 64) h.ep_len[ring + (size_t)((open + k) % cap)] = (int32_t)len;
    open = w;
  }
  if (lane == 0) {
    h.w[e] = w; h.tail[e] = tail; h.open[e] = open;
    if (counts) counts[e] = open - tail;
  }
}

// grid = n_envs blocks of one wavefront; mask null: every env
__global__ __launch_bounds__(64) void hrg_her_observe_kernel(const hrg_her_desc p, const HerDev h, const float* __restrict__ obs, const uint8_t* __restrict__ mask,
                                                             int64_t* __restrict__ counts) {
  const int e = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (e >= p.n_envs) return;
  if (!mask || mask[e]) {
    tracker_start(h.ep, e, lane, obs);
    if (lane == 0) h.w[e] = h.open[e];   // the slots of the unfinished episode are written again
  }
  if (lane == 0 && counts) counts[e] = h.open[e] - h.tail[e];
}

// One sample as its wavefront holds it: what both sample kernels store.
struct HerSample {
  float pre, post;    // column `lane` of the row before the step and of the row after it
  float goal;         // lane d < dg_dim: component d of the desired goal, stored or relabelled
  float v0, v1;       // value `lane` of the observation entry of both rows (zero past n_obs_cols), the goal columns rewritten with relabel_observation
  float rew;
  bool dn, relabel;
  int e;              // the env
  int64_t i, g;       // write counter of the transition, of the transition the new goal came from (-1: not relabelled)
  size_t s;           // the transition's slot
};

// Sample k of call `call`: the draws, the transition, the relabelling, reward and done.  N = cum[n_envs] > 0.  Every lane of the wave takes part (the shuffles).
DI HerSample her_draw(const hrg_her_desc& p, const HerDev& h, const int64_t* __restrict__ cum, int64_t N, uint64_t call, int k, int lane) {
  HerSample o;
  const double u0 = rng_u01(p.seed, call, (uint64_t)k, STREAM_HER, 0), u1 = rng_u01(p.seed, call, (uint64_t)k, STREAM_HER, 1), u2 = rng_u01(p.seed, call, (uint64_t)k, STREAM_HER, 2);
  const int64_t j = min((int64_t)floor(u0 * (double)N), N - 1);
  int lo = 0, hi = p.n_envs;   // the env with cum[e] <= j < cum[e + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cum[mid] <= j) lo = mid; else hi = mid;
  }
  const int e = lo;
  const int64_t cap = p.capacity;
  const size_t ring = (size_t)e * (size_t)cap;
  const int64_t tail = h.tail[e], closed = h.open[e] - tail;
  const int64_t i = tail + min(max(j - cum[e], (int64_t)0), max(closed - 1, (int64_t)0));   // (clamped: `cum` is the caller's)
  const size_t s = ring + (size_t)(i % cap);
  const int64_t es = h.ep_start[s];
  const int64_t L = max((int64_t)h.ep_len[s], (int64_t)1), t = min(max(i - es, (int64_t)0), L - 1);
  const bool relabel = u1 < p.her_ratio;
  int64_t f = L - 1;   // HRG_HER_FINAL
  if (p.strategy == HRG_HER_FUTURE) f = t + min((int64_t)floor(u2 * (double)(L - t)), L - t - 1);
  else if (p.strategy == HRG_HER_EPISODE) f = min((int64_t)floor(u2 * (double)L), L - 1);
  const float pre = h.pre[s * HRG_OBS_DIM + lane], post = h.post[s * HRG_OBS_DIM + lane];
  const int kind = p.goal_kind, na = her_ag_dim(kind), ng = her_dg_dim(kind);
  // the goal of lane d < ng: the stored desired goal, or what the transition `f` of the episode reached
  float goal = __shfl(pre, her_dg_col(kind, lane < ng ? lane : 0));
  float rew = h.reward[s];
  bool dn = h.done[s] != 0 && h.trunc[s] == 0;   // custom_add 52-58: a timeout is no termination
  if (relabel) {
    const float grow = h.post[(ring + (size_t)((es + f) % cap)) * HRG_OBS_DIM + lane];
    goal = __shfl(grow, her_new_goal_col(kind, lane < ng ? lane : 0));
    double a[7], g[6];
#pragma unroll
    for (int d = 0; d < 7; d++) a[d] = d < na ? (double)__shfl(post, her_ag_col(kind, d)) : 0.0;
#pragma unroll
    for (int d = 0; d < 6; d++) g[d] = d < ng ? (double)__shfl(goal, d) : 0.0;
    goal_reward_done(p, a, g, h.ctype[s], &rew, &dn);
  }
  // the policy's view of both rows: value `lane` of the observation entry (n_obs_cols <= 64); every lane takes part in the shuffles
  float v0 = view_select(h.view, pre, lane), v1 = view_select(h.view, post, lane);   // (entries past n_obs_cols are zero)
  if (relabel && p.relabel_observation) {   // (wave-uniform)
#pragma unroll
    for (int d = 0; d < 6; d++) {
      const float gd = __shfl(goal, d);
      if (d < p.n_dg_in_obs && lane == p.dg_in_obs[d]) v0 = v1 = gd;
    }
  }
  o.pre = pre; o.post = post; o.goal = goal; o.v0 = v0; o.v1 = v1; o.rew = rew; o.dn = dn; o.relabel = relabel;
  o.e = e; o.i = i; o.g = relabel ? es + f : -1; o.s = s;
  return o;
}

// what both sample kernels store once per sample: the action (lanes < act_dim), reward, done and the optional index row (lane 0)
DI void her_store_scalars(const hrg_her_desc& p, const HerDev& h, const HerSample& x, int k, int lane, float* __restrict__ o_act, float* __restrict__ o_rew,
                          float* __restrict__ o_done, int64_t* __restrict__ o_idx) {
  if (lane < p.act_dim) o_act[(size_t)k * p.act_dim + lane] = h.act[x.s * (size_t)p.act_dim + lane];
  if (lane == 0) {
    o_rew[k] = x.rew;
    o_done[k] = x.dn ? 1.0f : 0.0f;
    if (o_idx) { o_idx[(size_t)k * HRG_HER_INDEX_DIM] = x.e; o_idx[(size_t)k * HRG_HER_INDEX_DIM + 1] = x.i; o_idx[(size_t)k * HRG_HER_INDEX_DIM + 2] = x.g; }
  }
}

// grid = ceil(batch / 4) blocks of four wavefronts, one sample each.  `cum`: [n_envs + 1] exclusive prefix sums of the envs' closed transitions.
__global__ __launch_bounds__(HRG_BUFFER_BLOCK) void hrg_her_sample_kernel(const hrg_her_desc p, const HerDev h, const int64_t* __restrict__ cum, uint64_t call, int batch,
                                                                       float* __restrict__ o_obs, float* __restrict__ o_ag, float* __restrict__ o_dg,
                                                                       float* __restrict__ o_nobs, float* __restrict__ o_nag, float* __restrict__ o_ndg,
                                                                       float* __restrict__ o_act, float* __restrict__ o_rew, float* __restrict__ o_done,
                                                                       int64_t* __restrict__ o_idx) {
  const int lane = (int)(threadIdx.x & 63);
  const int k = buffer_wave_item();
  if (k >= batch) return;
  const int64_t N = cum[p.n_envs];
  if (N <= 0) return;   // (the host refuses the call)
  const HerSample x = her_draw(p, h, cum, N, call, k, lane);
  const int kind = p.goal_kind, na = her_ag_dim(kind), ng = her_dg_dim(kind);
  if (lane < p.n_obs_cols) {
    o_obs[(size_t)k * p.n_obs_cols + lane] = x.v0;
    o_nobs[(size_t)k * p.n_obs_cols + lane] = x.v1;
  }
  const float ag0 = __shfl(x.pre, her_ag_col(kind, lane < na ? lane : 0)), ag1 = __shfl(x.post, her_ag_col(kind, lane < na ? lane : 0));
  if (lane < na) { o_ag[(size_t)k * na + lane] = ag0; o_nag[(size_t)k * na + lane] = ag1; }
  if (lane < ng) { o_dg[(size_t)k * ng + lane] = x.goal; o_ndg[(size_t)k * ng + lane] = x.goal; }
  her_store_scalars(p, h, x, k, lane, o_act, o_rew, o_done, o_idx);
}

// Value `lane` of the feature row achieved_goal | desired_goal | observation (F = na + ng + n_obs_cols <= 64; zero past F).  row: column `lane` of the row of
// the superset, goal: component `lane` < ng of the desired goal, v: value `lane` of the observation entry.  Every lane of the wave takes part (the shuffles).
DI float her_feature(int kind, int n_obs_cols, float row, float goal, float v, int lane) {
  const int na = her_ag_dim(kind), ng = her_dg_dim(kind);
  const float a = __shfl(row, her_ag_col(kind, lane < na ? lane : 0));
  const float g = __shfl(goal, min(max(lane - na, 0), ng - 1));
  const float o = __shfl(v, min(max(lane - na - ng, 0), 63));   // value j of the observation entry moves from lane j to lane na + ng + j
  return lane < na ? a : lane < na + ng ? g : lane < na + ng + n_obs_cols ? o : 0.0f;
}

// grid = ceil(batch / 4) blocks of four wavefronts, one sample each; F <= HRG_OBS_DIM (the host checks).  Outputs are left unwritten where cum[n_envs] <= 0.
__global__ __launch_bounds__(HRG_BUFFER_BLOCK) void hrg_her_sample_features_kernel(const hrg_her_desc p, const HerDev h, const int64_t* __restrict__ cum, uint64_t call,
                                                                                int batch, float* __restrict__ o_feat, float* __restrict__ o_nfeat,
                                                                                float* __restrict__ o_act, float* __restrict__ o_rew, float* __restrict__ o_done,
                                                                                int64_t* __restrict__ o_idx) {
  const int lane = (int)(threadIdx.x & 63);
  const int k = buffer_wave_item();
  if (k >= batch) return;
  const int64_t N = cum[p.n_envs];
  if (N <= 0) return;   // (the caller checks once per train call)
  const HerSample x = her_draw(p, h, cum, N, call, k, lane);
  const int kind = p.goal_kind, F = her_ag_dim(kind) + her_dg_dim(kind) + p.n_obs_cols;
  const float f0 = her_feature(kind, p.n_obs_cols, x.pre, x.goal, x.v0, lane), f1 = her_feature(kind, p.n_obs_cols, x.post, x.goal, x.v1, lane);
  if (lane < F) {
    o_feat[(size_t)k * F + lane] = f0;
    o_nfeat[(size_t)k * F + lane] = f1;
  }
  her_store_scalars(p, h, x, k, lane, o_act, o_rew, o_done, o_idx);
}

// grid = ceil(n_rows / 4) blocks of four wavefronts, one row each; F <= HRG_OBS_DIM (the host checks)
__global__ __launch_bounds__(HRG_BUFFER_BLOCK) void hrg_her_features_kernel(const BufferView w, int kind, const float* __restrict__ rows, int n_rows, float* __restrict__ out) {
  const int lane = (int)(threadIdx.x & 63);
  const int r = buffer_wave_item();
  if (r >= n_rows) return;   // (wave-uniform)
  const int ng = her_dg_dim(kind), F = her_ag_dim(kind) + ng + w.n_obs_cols;
  const float x = rows[(size_t)r * HRG_OBS_DIM + lane];
  const float goal = __shfl(x, her_dg_col(kind, lane < ng ? lane : 0));
  const float f = her_feature(kind, w.n_obs_cols, x, goal, view_select(w, x, lane), lane);
  if (lane < F) out[(size_t)r * F + lane] = f;
}
