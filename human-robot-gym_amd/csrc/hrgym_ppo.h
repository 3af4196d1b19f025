// hrgym_ppo.h -- one minibatch step of PPO on the device: [UPSTREAM] stable-baselines3 1.5.0 PPO.train and ActorCriticPolicy for MlpPolicy, use_sde = False and Box
// actions (written out from knowledge of that release; the package is not a dependency), with hidden layers of width 64 and tanh units, depth 1 .. 3, plus the
// policy's and the value function's forward pass as the two callables HipVecEnv.collect_rollout takes.  Included into the base translation unit only
// (hrgym_hip.hip, HRG_BASE_TU), after hrgym_mlp.h: the networks are its tile products with tanh units, and its rules hold here (no vendor BLAS, no autograd, no
// atomics, a fixed order of every sum).
//
// One step is four launches (hrg_ppo_step), three without normalize_advantage:
//   1 hrg_ppo_adv_kernel     one workgroup: the minibatch's advantage mean and unbiased standard deviation (torch's), two passes.
//   2 hrg_ppo_grad_kernel    grid (tiles, networks): forward, the row's loss terms and their gradients at the heads' outputs, backward -> this tile's part of the
//                            gradient and of the loss sums.  Shared trunk: one network, the two heads are one [A + 1][64] product.  Separate trunks: network 0 is
//                            the policy (action_net, log_std), network 1 the value function (value_net).
//   3 hrg_ppo_reduce_kernel  grad = the tiles' parts summed in tile order; the squared norm of each block of 256 entries.
//   4 hrg_ppo_adam_kernel    the norm from the blocks' squares in block order, clip_grad_norm_'s coefficient min(1, max_grad_norm / (norm + 1e-6)) over ALL
//                            parameters, torch's Adam with PPO's eps = 1e-5 (betas 0.9, 0.999; bias corrections from the host), the diagnostics.
//
// A row's terms ([UPSTREAM] PPO.train; DiagGaussianDistribution, no squash), in double from the float32 head outputs, rounded once where stored:
//   log_prob = sum_j [-(a_j - mu_j)^2 / (2 exp(2 log_std_j)) - log_std_j - 0.5 log 2 pi],   entropy = sum_j (0.5 + 0.5 log 2 pi + log_std_j)
//   adv      = normalize_advantage ? (adv - mean) / (std + 1e-8) : adv
//   ratio    = exp(log_prob - old_log_prob),   policy_loss = -mean(min(adv ratio, adv clamp(ratio, 1 - c, 1 + c)))
//   vpred    = clip_range_vf ? old_value + clamp(value - old_value, -cv, cv) : value,   value_loss = mean((return - vpred)^2)
//   loss     = policy_loss + ent_coef (-mean(entropy)) + vf_coef value_loss
// The gradient of min(.,.) follows torch: where the ratio lies inside [1 - c, 1 + c] both arguments are equal and the two halves add up to the whole; outside, the
// clamp passes nothing, and the unclipped argument passes when it is the smaller one.
//
// The tiles' parts of a weight gradient are summed in tile order in the reduce kernel; the norm sums a block's 256 squares as a fixed tree and the blocks
// ascending.  With hrgym_mlp.h's orders that fixes every sum: two learners fed the same minibatches end bit-identical.
//
// Parameters (float32, flat, allocated by the caller; torch's [out][in] weight layout).  in_0 = K, in = 64 afterwards:
//   network n (one when shared, policy | value when separate): for l < depth: W_l [64][in_l], b_l [64]
//   heads   : W_action [A][64], W_value [1][64], b_action [A], b_value [1]
//   log_std : [A]
//
// Draws of the forward pass: rng_gauss keyed by (learner seed, forward call count, row, STREAM_PPO_ACT, component); none depends on the grid.
//
// A population is n_members learners of one shape that step in the same four launches: blockIdx.z = p is the member.  They differ in their seed
// and, where the caller set them (hrg_ppo_population_set_hyper), in their row of the hyper-parameter table: learning rate, the two clip ranges, ent_coef, vf_coef,
// max_grad_norm (PpoHyper).  A kernel reads its member's row once per workgroup, an address every lane shares, and uses the values as the lone learner does.
// Parameters and moments are [P][n_params], the batch arrays [P][B][.], every piece of the handle's scratch has a member stride (ppo_member), the seeds are a [P]
// table.  The counters are the handle's: members step in lockstep.  A member's advantage statistics, clip coefficient and diagnostics come from its own sums, its
// draws are keyed by its own seed and the row's index in its group of rows: member p is, bit for bit, the lone learner of seed p and row p on batch p.  The lone learner is
// the population of one member.
#pragma once

enum { STREAM_PPO_ACT = 14 };   // after STREAM_SAC_ACT = 13 (hrgym_sac.h)
#define PPO_NPART 6   // per tile: sum of -min(.,.), of (ratio - 1) - log ratio, of [|ratio - 1| > c], of (return - vpred)^2; a row's entropy; mean_j exp(log_std_j)

// a member's row of the handle's hyper-parameter table (include/hrgym.h: hrg_ppo_hyper, in the types the kernels compute with)
struct PpoHyper {
  double lr = 0.0, clip_range = 0.0, clip_range_vf = -1.0;   // (negative: the value function is not clipped)
  float ent_coef = 0.0f, vf_coef = 0.0f, max_grad_norm = 0.0f;
  int32_t reserved = 0;   // (no padding: the host compares rows as bytes)
};
static_assert(sizeof(PpoHyper) == 40, "no padding in a row of the PPO hyper-parameter table");

// a member's pieces of the scratch the handle owns
struct PpoScratch {
  float* values = nullptr;     // [B]
  float* logp = nullptr;       // [B]
  float* ratio = nullptr;      // [B]
  float* part = nullptr;       // [tiles][n_params] the tiles' parts of the gradient
  float* grad = nullptr;       // [n_params] their sum (the last step's gradient, before clipping)
  float* loss_part = nullptr;  // [tiles][PPO_NPART]
  float* diag = nullptr;       // [HRG_PPO_NDIAG]
  double* adv_stat = nullptr;  // [2] mean, std of the minibatch's advantages
  double* block_sq = nullptr;  // [ceil(n_params / 256)]
};

// one hrg_ppo: sizes, offsets into the parameter vector, the scratch it owns; passed to the kernels by value
struct PpoDev {
  int32_t K = 0, A = 0, depth = 0, B = 0, tiles = 0, n_params = 0, nets = 0, normalize = 0;
  int32_t w[2][HRG_PPO_MAX_DEPTH] = {{0}}, b[2][HRG_PPO_MAX_DEPTH] = {{0}}, hw = 0, hb = 0, ls = 0;   // the networks' layers; the heads' [A + 1][64] weights and [A + 1] biases; log_std
  const PpoHyper* hyper = nullptr;   // [P] the members' hyper-parameters
  const uint64_t* seeds = nullptr;   // [P] the members' seeds
  PpoScratch all;                    // the scratch of every member, [P] pieces of each array: member 0's pointers
};

// member p's pieces of the scratch.  The kernels move the arrays they are passed themselves (mlp_rows).  (A copy of the pointers alone: a copy of the whole
// handle, whose offset tables the kernels index by the network, would live in scratch memory.)
DI PpoScratch ppo_member(const PpoDev& h, int p) {
  const size_t i = (size_t)p, B = (size_t)h.B, n = (size_t)h.n_params, tiles = (size_t)h.tiles;
  PpoScratch m = h.all;
  m.values += i * B;
  m.logp += i * B;
  m.ratio += i * B;
  m.part += i * tiles * n;
  m.grad += i * n;
  m.loss_part += i * tiles * PPO_NPART;
  m.diag += i * HRG_PPO_NDIAG;
  m.adv_stat += i * 2;
  m.block_sq += i * ((n + MLP_BLOCK - 1) / MLP_BLOCK);
  return m;
}

// which outputs of the heads a workgroup computes: the first row of the [A + 1][64] product, the number of rows, the column of the value in s.D
struct PpoHead {
  int first, nout, vcol;
  bool pol, val;
};
DI PpoHead ppo_head(const PpoDev& h, int net, bool value_only) {
  PpoHead o;
  o.pol = !value_only && (h.nets == 1 || net == 0);
  o.val = value_only || h.nets == 1 || net == 1;
  o.first = o.pol ? 0 : h.A;
  o.nout = (o.pol ? h.A : 0) + (o.val ? 1 : 0);
  o.vcol = o.pol ? h.A : 0;
  return o;
}

// sum of x[0 .. n) for the whole workgroup: thread t takes t, t + 256, .. ascending, thread 0 adds the 256 partial sums ascending.  Ends with a barrier.
DI double ppo_block_sum(double* red, double mine) {
  red[threadIdx.x] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    double sum = 0.0;
    for (int i = 0; i < MLP_BLOCK; i++) sum += red[i];
    red[MLP_BLOCK] = sum;
  }
  __syncthreads();
  const double out = red[MLP_BLOCK];
  __syncthreads();
  return out;
}

// ---- 1: mean and unbiased standard deviation of the minibatch's advantages.  Grid (1, 1, members).
__global__ __launch_bounds__(MLP_BLOCK) void hrg_ppo_adv_kernel(const PpoDev h, const float* __restrict__ adv) {
  __shared__ double red[MLP_BLOCK + 1];
  const int t = (int)threadIdx.x, p = (int)blockIdx.z;
  const PpoScratch m = ppo_member(h, p);
  adv = mlp_rows(adv, p, (size_t)h.B);
  double sum = 0.0;
  for (int i = t; i < h.B; i += MLP_BLOCK) sum += (double)adv[i];
  const double mean = ppo_block_sum(red, sum) / (double)h.B;
  double sq = 0.0;
  for (int i = t; i < h.B; i += MLP_BLOCK) sq += ((double)adv[i] - mean) * ((double)adv[i] - mean);
  const double var = ppo_block_sum(red, sq) / (double)(h.B - 1);
  if (t == 0) {
    m.adv_stat[0] = mean;
    m.adv_stat[1] = sqrt(var);
  }
}

// ---- 2: network blockIdx.y of member blockIdx.z on the tile: forward, the rows' losses and their gradients at the heads, backward
__global__ __launch_bounds__(MLP_BLOCK) void hrg_ppo_grad_kernel(const PpoDev h, const float* __restrict__ P, const float* __restrict__ obs, const float* __restrict__ act,
                                                                 const float* __restrict__ old_values, const float* __restrict__ old_logp, const float* __restrict__ adv,
                                                                 const float* __restrict__ returns) {
  __shared__ MlpLds s;
  const int row0 = (int)blockIdx.x * MLP_T, net = (int)blockIdx.y, p = (int)blockIdx.z, K = h.K, A = h.A, t = (int)threadIdx.x;
  if (row0 >= h.B) return;   // (uniform over the workgroup)
  const PpoScratch m = ppo_member(h, p);
  const PpoHyper hy = h.hyper[p];
  const double clip_range = hy.clip_range, clip_range_vf = hy.clip_range_vf;
  const size_t B = (size_t)h.B;
  P = mlp_rows(P, p, (size_t)h.n_params); obs = mlp_rows(obs, p, B * K); act = mlp_rows(act, p, B * A);
  old_values = mlp_rows(old_values, p, B); old_logp = mlp_rows(old_logp, p, B); adv = mlp_rows(adv, p, B); returns = mlp_rows(returns, p, B);
  const PpoHead hd = ppo_head(h, net, false);
  const int hw = h.hw + hd.first * MLP_H, hb = h.hb + hd.first;
  float* part = m.part + (size_t)blockIdx.x * h.n_params;
  mlp_load(s, obs, K, 0, row0, h.B);
  mlp_trunk(s, P, h.w[net], h.b[net], h.depth, K, MLP_ACT_TANH);
  mlp_head(s, P, hw, hb, h.depth, hd.nout);
  const double inv_b = 1.0 / (double)h.B;
  for (int r = t; r < MLP_T; r += (int)blockDim.x) {
    const int i = row0 + r;
    if (hd.val) {
      const float v = s.D[r * MLP_DLD + hd.vcol], ov = old_values[i];
      const double dv = (double)v - (double)ov;
      const bool clip = clip_range_vf >= 0.0, pass = !clip || (dv >= -clip_range_vf && dv <= clip_range_vf);
      const double vp = clip ? (double)ov + fmin(fmax(dv, -clip_range_vf), clip_range_vf) : (double)v, d = vp - (double)returns[i];
      m.values[i] = v;
      s.row[3][r] = (float)(d * d);
      s.D[r * MLP_DLD + hd.vcol] = pass ? (float)((double)hy.vf_coef * 2.0 * d * inv_b) : 0.0f;
    }
    if (hd.pol) {
      double lp = 0.0;
      for (int j = 0; j < A; j++) {
        const double ls = (double)P[h.ls + j], d = (double)act[(size_t)i * A + j] - (double)s.D[r * MLP_DLD + j];
        lp += -0.5 * d * d * exp(-2.0 * ls) - ls - MLP_HALF_LOG_2PI;
      }
      const double log_ratio = lp - (double)old_logp[i], ratio = exp(log_ratio), c = clip_range;
      const double a = h.normalize ? ((double)adv[i] - m.adv_stat[0]) / (m.adv_stat[1] + 1e-8) : (double)adv[i];
      const bool inside = ratio >= 1.0 - c && ratio <= 1.0 + c;
      const double s1 = a * ratio, s2 = a * fmin(fmax(ratio, 1.0 - c), 1.0 + c);
      const double g = (inside || s1 < s2) ? -a * ratio * inv_b : 0.0;   // d loss / d log_prob
      for (int j = 0; j < A; j++) {
        const double ls = (double)P[h.ls + j], iv = exp(-2.0 * ls), d = (double)act[(size_t)i * A + j] - (double)s.D[r * MLP_DLD + j];
        s.D[r * MLP_DLD + j] = (float)(g * d * iv);                                          // ... / d mu_j
        s.std[r * 8 + j] = (float)(g * (d * d * iv - 1.0) - (double)hy.ent_coef * inv_b);     // ... / d log_std_j, with the entropy bonus's share of the row
      }
      m.logp[i] = (float)lp;
      m.ratio[i] = (float)ratio;
      s.row[0][r] = (float)(-fmin(s1, s2));
      s.row[1][r] = (float)((ratio - 1.0) - log_ratio);
      s.row[2][r] = fabs(ratio - 1.0) > c ? 1.0f : 0.0f;
    }
  }
  __syncthreads();
  if (t == 0) {
    float* lpart = m.loss_part + (size_t)blockIdx.x * PPO_NPART;
    for (int k = hd.pol ? 0 : 3; k < (hd.val ? 4 : 3); k++) {
      double sum = 0.0;
      for (int r = 0; r < MLP_T; r++) sum += (double)s.row[k][r];
      lpart[k] = (float)sum;
    }
    if (hd.pol) {
      double ent = 0.0, sd = 0.0;
      for (int j = 0; j < A; j++) {
        ent += 0.5 + MLP_HALF_LOG_2PI + (double)P[h.ls + j];
        sd += exp((double)P[h.ls + j]);
      }
      lpart[4] = (float)ent;
      lpart[5] = (float)(sd / (double)A);
    }
  }
  if (hd.pol && t >= 64 && t < 64 + A) {   // (a wave of its own: thread 0 is busy with the loss sums)
    double sum = 0.0;
    for (int r = 0; r < MLP_T; r++) sum += (double)s.std[r * 8 + (t - 64)];
    part[h.ls + t - 64] = (float)sum;
  }
  mlp_backward(s, P, h.w[net], h.b[net], hw, hb, h.depth, K, hd.nout, part, true, 0, MLP_ACT_TANH);
}

// ---- 3: the gradient (the tiles' parts in tile order) and each block's squared norm (a fixed tree over the block's 256 entries).  Grid (blocks, 1, members).
__global__ __launch_bounds__(MLP_BLOCK) void hrg_ppo_reduce_kernel(const PpoDev h) {
  __shared__ double red[MLP_BLOCK];
  const int t = (int)threadIdx.x, i = (int)(blockIdx.x * blockDim.x) + t;
  const PpoScratch m = ppo_member(h, (int)blockIdx.z);
  float g = 0.0f;
  if (i < h.n_params) {
    double sum = 0.0;
    for (int tl = 0; tl < h.tiles; tl++) sum += (double)m.part[(size_t)tl * h.n_params + i];
    g = (float)sum;
    m.grad[i] = g;
  }
  red[t] = (double)g * (double)g;
  __syncthreads();
  for (int w = MLP_BLOCK / 2; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  if (t == 0) m.block_sq[blockIdx.x] = red[0];
}

// ---- 4: clip_grad_norm_ over all parameters, torch's Adam (eps 1e-5) in double, rounded once into the float32 parameter; thread 0 of block 0: the diagnostics.
// Grid (blocks, 1, members): the norm, the coefficient and the tail are the member's own.
__global__ __launch_bounds__(MLP_BLOCK) void hrg_ppo_adam_kernel(const PpoDev h, float* __restrict__ P, float* __restrict__ M, float* __restrict__ V, int n_blocks,
                                                                 double bc1, double bc2) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x), p = (int)blockIdx.z;
  const PpoScratch own = ppo_member(h, p);   // (`m` is Adam's first moment below)
  const PpoHyper hy = h.hyper[p];
  const double lr = hy.lr;
  P = mlp_rows(P, p, (size_t)h.n_params); M = mlp_rows(M, p, (size_t)h.n_params); V = mlp_rows(V, p, (size_t)h.n_params);
  double sq = 0.0;
  for (int b = 0; b < n_blocks; b++) sq += own.block_sq[b];
  const double norm = sqrt(sq), coef = fmin(1.0, (double)hy.max_grad_norm / (norm + 1e-6));
  if (i < h.n_params) {   // (mlp_adam's update written out: through the helper the compiler contracts v's products the other way round, a different rounding)
    const double gd = (double)own.grad[i] * coef, m = 0.9 * (double)M[i] + 0.1 * gd, v = 0.999 * (double)V[i] + 0.001 * gd * gd;
    P[i] = (float)((double)P[i] - lr * (m / bc1) / (sqrt(v / bc2) + 1e-5));
    M[i] = (float)m;
    V[i] = (float)v;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    for (int tl = 0; tl < h.tiles; tl++)
      for (int k = 0; k < 4; k++) sum[k] += (double)own.loss_part[(size_t)tl * PPO_NPART + k];
    const double inv_b = 1.0 / (double)h.B, pl = sum[0] * inv_b, vl = sum[3] * inv_b, el = -(double)own.loss_part[4];
    own.diag[0] = (float)pl;                                                  // policy_gradient_loss
    own.diag[1] = (float)vl;                                                  // value_loss
    own.diag[2] = (float)el;                                                  // entropy_loss
    own.diag[3] = (float)(pl + (double)hy.ent_coef * el + (double)hy.vf_coef * vl);   // loss
    own.diag[4] = (float)(sum[1] * inv_b);                                    // approx_kl
    own.diag[5] = (float)(sum[2] * inv_b);                                    // clip_fraction
    own.diag[6] = own.loss_part[5];                                             // std
    own.diag[7] = (float)norm;                                                // the gradient norm before clipping
  }
}

// ---- the forward pass on any number of rows, a tile of rows per workgroup.  value_only = 0, grid (tiles, networks, members): actions = mu + exp(log_std) eps (not
// clipped; deterministic: mu), their log_prob, and the values.  value_only = 1, grid (tiles, 1, members): the values.  obs, eps_in and the outputs are [P][n][.],
// member blockIdx.z's networks on its group of n rows.  The tile's bound is the end of the group, and a draw's key the row's index in the group.
__global__ __launch_bounds__(MLP_BLOCK) void hrg_ppo_forward_kernel(const PpoDev h, const float* __restrict__ P, const float* __restrict__ obs, int n,
                                                                    const float* __restrict__ eps_in, int deterministic, uint64_t call, int value_only,
                                                                    float* __restrict__ actions, float* __restrict__ values, float* __restrict__ logp) {
  __shared__ MlpLds s;
  const int row0 = (int)blockIdx.x * MLP_T, net = value_only ? h.nets - 1 : (int)blockIdx.y, p = (int)blockIdx.z, K = h.K, A = h.A;
  if (row0 >= n) return;
  P = mlp_rows(P, p, (size_t)h.n_params); obs = mlp_rows(obs, p, (size_t)n * K); eps_in = mlp_rows_or_null(eps_in, p, (size_t)n * A);
  actions = mlp_rows_or_null(actions, p, (size_t)n * A); values = mlp_rows(values, p, (size_t)n); logp = mlp_rows_or_null(logp, p, (size_t)n);
  const PpoHead hd = ppo_head(h, net, value_only != 0);
  mlp_load(s, obs, K, 0, row0, n);
  if (hd.pol) {
    if (deterministic) {
      for (int i = (int)threadIdx.x; i < MLP_T * 8; i += (int)blockDim.x) s.eps[i] = 0.0f;
    } else {
      mlp_noise(s, eps_in, A, row0, n, h.seeds[p], call, STREAM_PPO_ACT, 0);
    }
  }
  mlp_trunk(s, P, h.w[net], h.b[net], h.depth, K, MLP_ACT_TANH);
  mlp_head(s, P, h.hw + hd.first * MLP_H, h.hb + hd.first, h.depth, hd.nout);
  for (int r = (int)threadIdx.x; r < MLP_T; r += (int)blockDim.x) {
    const int i = row0 + r;
    if (i >= n) continue;
    if (hd.val) values[i] = s.D[r * MLP_DLD + hd.vcol];
    if (hd.pol) {
      double lp = 0.0;
      for (int j = 0; j < A; j++) {
        const double ls = (double)P[h.ls + j], mu = (double)s.D[r * MLP_DLD + j];
        const float a = (float)(mu + exp(ls) * (double)s.eps[r * 8 + j]);   // the log_prob is that of the float32 action the buffer stores
        const double d = (double)a - mu;
        actions[(size_t)i * A + j] = a;
        lp += -0.5 * d * d * exp(-2.0 * ls) - ls - MLP_HALF_LOG_2PI;
      }
      logp[i] = (float)lp;
    }
  }
}
