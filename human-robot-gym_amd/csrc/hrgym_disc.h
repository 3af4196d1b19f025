// hrgym_disc.h -- adversarial imitation on the device (Ho & Ermon 2016, GAIL; Fu, Luo, Levine 2018, AIRL; off-policy as in Kostrikov et al. 2019): a discriminator
// D(obs, action) trained to tell the rows of a demonstration table from the learner's own rows, and the reward it gives a batch.  Included into the base translation
// unit only (hrgym_hip.hip, HRG_BASE_TU), after hrgym_dagger.h: the network is hrgym_mlp.h's tile products, and its rules hold here (no vendor BLAS, no autograd, no
// atomics, a fixed order of every sum).  The network has a SAC critic's shape: input [obs (K) | action (A)], `depth` hidden layers of 64 units (ReLU or tanh, a
// constant of the handle), a head of one output: the logit d that the row is the expert's.  Its parameters are a vector of its own, W_l [64][in_l], b_l [64] for
// l < depth, then W_d [1][64], b_d [1].
//
// One update is two launches (hrg_disc_step):
//   1 hrg_disc_grad_kernel  grid (2 B / 32 tiles): tiles 0 .. B / 32 - 1 hold expert rows -- the tile's table indices, drawn or supplied, the rows gathered straight
//                           from the table --, the rest row k of the caller's policy tensors.  Trunk and head forward; the loss and its gradient at the logit;
//                           backward -> this tile's part of the gradient, of the loss sum and of the two counts of rows on the right side of d = 0.
//   2 hrg_disc_adam_kernel  every entry: the tiles' parts summed in tile order, torch's Adam with eps 1e-8 (mlp_adam) on the handle's own step count; thread 0 of
//                           block 0 sums the loss and the accuracies.
// and the reward is one (hrg_disc_reward):
//     hrg_disc_reward_kernel  grid (ceil(n / 32) tiles), forward only, n >= 1 rows of the caller's; rows behind n are zero in the tile and store nothing.  It writes
//                           nothing of the discriminator's.
//
// The loss is binary cross-entropy on the logit, L = (1 / 2B) (sum_expert softplus(-d) + sum_policy softplus(d)), softplus(x) = max(x, 0) + log1p(exp(-|x|)) in
// double; its gradient at the logit (sigmoid(d) - y) / 2B in double, rounded once (y = 1 for an expert row).  The reward: softplus(d) = -log(1 - D) for
// HRG_DISC_REWARD_GAIL, d = log D - log(1 - D) for HRG_DISC_REWARD_AIRL, in double; with the env's rewards r_disc alpha + r_env (1 - alpha), hrg_sir_post_kernel's
// expression, rounded once.
//
// Draws: expert row k takes table row min(floor(u n_rows), n_rows - 1), u = rng_u01 keyed by (seed, step count, k, STREAM_DISC, 0): independent of the grid.  A
// supplied index is clamped into the table (the Python side raises IndexError before the launch).
#pragma once

enum { STREAM_DISC = 17 };   // after STREAM_DAGGER = 16 (hrgym_dagger.h)
#define DISC_NSTAT 3         // per tile: the loss sum, expert rows with d > 0, policy rows with d < 0

// one hrg_disc: the network's offsets, the scratch the handle owns; passed to the kernels by value
struct DiscDev {
  int32_t w[HRG_SAC_MAX_DEPTH] = {0}, b[HRG_SAC_MAX_DEPTH] = {0}, hw = 0, hb = 0;
  int32_t depth = 0, K = 0, A = 0, B = 0, tiles = 0, n_params = 0, unit = 0, kind = 0;   // B: rows per half; tiles = 2 B / 32; unit: MLP_ACT_RELU | MLP_ACT_TANH
  uint64_t seed = 0;
  int64_t* index = nullptr;         // [B] the last step's table rows
  float* logits = nullptr;          // [2 B] expert rows, then policy rows
  float* part = nullptr;            // [tiles][n_params] the tiles' parts of the gradient
  float* grad = nullptr;            // [n_params] their sum
  float* stat_part = nullptr;       // [tiles][DISC_NSTAT]
  float* diag = nullptr;            // [3] loss, expert accuracy, policy accuracy
};

DI double disc_softplus(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }

// ---- 1: the tile's rows (of the table, or the caller's), forward, the loss, backward
__global__ __launch_bounds__(MLP_BLOCK) void hrg_disc_grad_kernel(const DiscDev h, const float* __restrict__ P, const float* __restrict__ table_obs,
                                                                  const float* __restrict__ table_act, int64_t n_rows, const int64_t* __restrict__ index_in,
                                                                  const float* __restrict__ policy_obs, const float* __restrict__ policy_act, uint64_t count) {
  __shared__ MlpLds s;
  __shared__ int64_t rows[MLP_T];
  const int tile = (int)blockIdx.x, half = h.tiles >> 1, K = h.K, A = h.A, t = (int)threadIdx.x;
  if (tile >= h.tiles) return;   // (uniform over the workgroup)
  const bool expert = tile < half;
  const int row0 = (expert ? tile : tile - half) * MLP_T;   // within the half
  if (expert) {
    if (t < MLP_T) {
      const int k = row0 + t;
      int64_t i = index_in ? index_in[k] : (int64_t)floor(rng_u01(h.seed, count, (uint64_t)k, STREAM_DISC, 0) * (double)n_rows);
      i = min(max(i, (int64_t)0), n_rows - 1);   // (u < 1: the bound keeps a draw inside the table whatever the rounding)
      rows[t] = i;
      h.index[k] = i;
    }
    __syncthreads();
    for (int i = t; i < MLP_T * K; i += (int)blockDim.x) s.X[(i / K) * MLP_XLD + i % K] = table_obs[(size_t)rows[i / K] * K + i % K];
    for (int i = t; i < MLP_T * A; i += (int)blockDim.x) s.X[(i / A) * MLP_XLD + K + i % A] = table_act[(size_t)rows[i / A] * A + i % A];
  } else {
    mlp_load(s, policy_obs, K, 0, row0, h.B);
    mlp_load(s, policy_act, A, K, row0, h.B);
  }
  mlp_trunk(s, P, h.w, h.b, h.depth, K + A, h.unit);
  mlp_head(s, P, h.hw, h.hb, h.depth, 1);
  const double scale = 1.0 / (2.0 * (double)h.B);
  for (int r = t; r < MLP_T; r += (int)blockDim.x) {
    const float d = s.D[r * MLP_DLD];
    const double x = (double)d, sig = 1.0 / (1.0 + exp(-x));
    h.logits[tile * MLP_T + r] = d;
    s.row[0][r] = (float)disc_softplus(expert ? -x : x);
    s.row[1][r] = (expert ? d > 0.0f : d < 0.0f) ? 1.0f : 0.0f;
    s.D[r * MLP_DLD] = (float)((sig - (expert ? 1.0 : 0.0)) * scale);
  }
  __syncthreads();
  if (t == 0) {
    double sum = 0.0, right = 0.0;
    for (int r = 0; r < MLP_T; r++) {
      sum += (double)s.row[0][r];
      right += (double)s.row[1][r];
    }
    float* st = h.stat_part + (size_t)tile * DISC_NSTAT;
    st[0] = (float)sum;
    st[1] = expert ? (float)right : 0.0f;
    st[2] = expert ? 0.0f : (float)right;
  }
  mlp_backward(s, P, h.w, h.b, h.hw, h.hb, h.depth, K + A, 1, h.part + (size_t)tile * h.n_params, true, 0, h.unit);
}

// ---- 2: entry i: the gradient (the tiles' parts in tile order, in double, rounded once), torch's Adam with eps 1e-8; thread 0 of block 0: the loss and the
// accuracies.  Grid = blocks of 256 over n_params.
__global__ __launch_bounds__(MLP_BLOCK) void hrg_disc_adam_kernel(const DiscDev h, float* __restrict__ P, float* __restrict__ M, float* __restrict__ V, double lr,
                                                                  double bc1, double bc2) {
  const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (e < h.n_params) {
    double sum = 0.0;
    for (int tl = 0; tl < h.tiles; tl++) sum += (double)h.part[(size_t)tl * h.n_params + e];
    const float g = (float)sum;
    h.grad[e] = g;
    mlp_adam(P, M, V, e, (double)g, lr, bc1, bc2, 1e-8);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double sum[DISC_NSTAT] = {0.0, 0.0, 0.0};
    for (int tl = 0; tl < h.tiles; tl++)
      for (int j = 0; j < DISC_NSTAT; j++) sum[j] += (double)h.stat_part[(size_t)tl * DISC_NSTAT + j];
    h.diag[0] = (float)(sum[0] / (2.0 * (double)h.B));
    h.diag[1] = (float)(sum[1] / (double)h.B);
    h.diag[2] = (float)(sum[2] / (double)h.B);
  }
}

// ---- the reward of n rows: forward only.  env_rewards (or null) and rewards_out may be one array: a row is read and written by one thread.  logits_out may be
// null.
__global__ __launch_bounds__(MLP_BLOCK) void hrg_disc_reward_kernel(const DiscDev h, const float* __restrict__ P, const float* __restrict__ obs,
                                                                    const float* __restrict__ act, int n, const float* env_rewards, double alpha, float* rewards_out,
                                                                    float* __restrict__ logits_out) {
  __shared__ MlpLds s;
  const int row0 = (int)blockIdx.x * MLP_T, K = h.K, A = h.A, t = (int)threadIdx.x;
  if (row0 >= n) return;   // (uniform over the workgroup)
  mlp_load(s, obs, K, 0, row0, n);
  mlp_load(s, act, A, K, row0, n);
  mlp_trunk(s, P, h.w, h.b, h.depth, K + A, h.unit);
  mlp_head(s, P, h.hw, h.hb, h.depth, 1);
  for (int r = t; r < MLP_T; r += (int)blockDim.x) {
    if (row0 + r >= n) continue;   // the ragged last tile
    const float d = s.D[r * MLP_DLD];
    const double r_disc = h.kind == HRG_DISC_REWARD_GAIL ? disc_softplus((double)d) : (double)d;
    if (logits_out) logits_out[row0 + r] = d;
    if (rewards_out) rewards_out[row0 + r] = env_rewards ? (float)(r_disc * alpha + (double)env_rewards[row0 + r] * (1.0 - alpha)) : (float)r_disc;
  }
}
