// hrgym_sac.h -- one gradient step of SAC on the device: [UPSTREAM] stable-baselines3 1.5.0 SAC.train for use_sde = False (written out from knowledge of that
// release; the package is not a dependency) with MlpPolicy networks of hidden width 64 and depth 1 .. 3, plus the actor's forward pass as the `policy` that
// HipVecEnv.collect_steps takes.  Included into the base translation unit only (hrgym_hip.hip, HRG_BASE_TU), after hrgym_mlp.h: the networks are its tile
// products with ReLU units, and its rules hold here (no vendor BLAS, no autograd, no atomics, a fixed order of every sum).
//
// One step is six launches (hrg_sac_step):
//   1 hrg_sac_policy_kernel   grid (tiles, 2).  y = 0: the actor on `obs` with eps_pi -> a_pi, logp.  y = 1: the actor on `next_obs` with eps_next -> a', logp',
//                             the two TARGET critics on (next_obs, a') -> y = r + (1 - d) gamma (min(Q1t, Q2t) - alpha logp').
//   2 hrg_sac_critic_kernel   grid (tiles, 2): critic c on (obs, act), d loss / d q = (q - y) / B, backward -> this tile's part of the critic's gradient.
//   3 hrg_sac_adam_kernel     the critics' parameters: the tiles' parts summed in tile order, Adam, and the polyak update of the targets when it is due.
//   4 hrg_sac_actor_q_kernel  grid (tiles, 2): the UPDATED critic c on (obs, a_pi) -> q and d q / d a (backward to the action columns of the input only).
//   5 hrg_sac_actor_kernel    grid (tiles): the actor on `obs` again (the same values as in 1: the actor has not moved), d loss / d mu, d loss / d log_std of
//                             mean(alpha logp - min(Q1, Q2)), backward -> this tile's part of the actor's gradient.
//   6 hrg_sac_adam_kernel     the actor's parameters, and the entropy coefficient's gradient -mean(logp + target_entropy) with its Adam step when it is learned.
// alpha = exp(log_ent_coef) is read in 1 and 5, the coefficient moves in 6: every use in a step sees the value from before the step's update.
//
// The batch is at most 256 rows: 1 .. 8 tiles.  The tiles' parts of a weight gradient are summed in tile order in the Adam kernel.
//
// What differs from SB3: the draws (rng_gauss below, not torch's generator), the summation order, the transcendentals (-fapprox-func: expf, logf, tanhf are
// within a few ulps and are kept out of the
// squash: tanh, exp, log and the row's logp and its gradient are evaluated in double, a few values per row), Adam's update computed in double and rounded
// once into the float32 parameter.
//
// Parameters (float32, flat, allocated by the caller; torch's [out][in] weight layout).  in0 = K for the actor, K + A for a critic; in = 64 afterwards:
//   actor   : for l < depth: W_l [64][in_l], b_l [64];  W_mu [A][64], W_log_std [A][64], b_mu [A], b_log_std [A]     (the two heads are one [2A][64] product)
//   critic c: for l < depth: W_l [64][in_l], b_l [64];  W_q [1][64], b_q [1]
//   params  = actor | critic 0 | critic 1 | log_ent_coef;   adam_m, adam_v: the same layout;   target = critic 0 | critic 1.
//
// Draws: rng_gauss keyed by (learner seed, gradient step count, batch row, STREAM_SAC, component), component j for eps_pi and HRG_ACT_DIM + j for eps_next; the
// act kernel by (seed, act call count, row, STREAM_SAC_ACT, j).  None depends on the grid.
//
// A population is n_members learners of one shape that step in the same six launches: blockIdx.z = p is the member (the act kernel:
// blockIdx.y).  They differ in their seed and, where the caller set them (hrg_sac_population_set_hyper), in their row of the hyper-parameter table: learning rate,
// gamma, tau, target entropy, the entropy coefficient's fixed value and whether it is learned (SacHyper).  A kernel reads its member's row once per workgroup, an
// address every lane shares, and uses the values as the lone learner does: the same types, the same order.  Parameters, moments and targets are [P][n_params] and [P][2 n_critic], the batch arrays [P][B][.], every piece of the handle's
// scratch has a member stride (sac_member), the seeds are a [P] table.  The counters are the handle's: members step in lockstep.  A member's draws are keyed by its
// own seed and the row's index in its own batch (the act kernel: in its group of rows), its sums are its own: member p is, bit for bit, the lone learner of seed p
// and row p on batch p.  The lone learner is the population of one member.
#pragma once

enum { STREAM_SAC = 12, STREAM_SAC_ACT = 13 };   // after STREAM_REPLAY = 11 (hrgym_replay.h)
#define SAC_NQ HRG_SAC_NQ   // Q columns kept for the export: Q1, Q2 on (obs, act); Q1t, Q2t on (next_obs, a'); Q1, Q2 (updated) on (obs, a_pi)
#define SAC_NLOSS 4       // per tile: sum (Q1 - y)^2, sum (Q2 - y)^2, sum (alpha logp - min Q), sum logp

// a member's row of the handle's hyper-parameter table (include/hrgym.h: hrg_sac_hyper, in the types the kernels compute with)
struct SacHyper {
  double lr = 0.0, tau = 0.0;
  float gamma = 0.0f, alpha_fixed = 0.0f, target_entropy = 0.0f;
  int32_t auto_alpha = 0;
};
static_assert(sizeof(SacHyper) == 32, "no padding in a row of the SAC hyper-parameter table: the host compares rows as bytes");

// a member's seed and its pieces of the scratch the handle owns
struct SacScratch {
  uint64_t seed = 0;
  float* a_pi = nullptr;       // [B][A]
  float* logp = nullptr;       // [B]
  float* logp_next = nullptr;  // [B]
  float* y = nullptr;          // [B]
  float* q = nullptr;          // [SAC_NQ][B]
  float* dqda = nullptr;       // [2][B][A]
  float* part = nullptr;       // [tiles][n_params] the tiles' parts of the gradient
  float* grad = nullptr;       // [n_params] their sum (the last step's gradient)
  float* loss_part = nullptr;  // [tiles][SAC_NLOSS]
  float* losses = nullptr;     // [4] actor_loss, critic_loss, ent_coef_loss, ent_coef (the alpha the step used)
};

// one hrg_sac: sizes, offsets into the parameter vector, the scratch it owns; passed to the kernels by value
struct SacDev {
  int32_t K = 0, A = 0, depth = 0, B = 0, tiles = 0, n_params = 0, n_actor = 0, n_critic = 0;
  int32_t a_w[HRG_SAC_MAX_DEPTH] = {0}, a_b[HRG_SAC_MAX_DEPTH] = {0}, a_hw = 0, a_hb = 0;   // actor: hidden layers, the heads' [2A][64] weights and [2A] biases
  int32_t q_w[2][HRG_SAC_MAX_DEPTH] = {{0}}, q_b[2][HRG_SAC_MAX_DEPTH] = {{0}}, q_ow[2] = {0}, q_ob[2] = {0};
  const SacHyper* hyper = nullptr;   // [P] the members' hyper-parameters
  const uint64_t* seeds = nullptr;   // [P] the members' seeds
  SacScratch all;                    // the scratch of every member, [P] pieces of each array: member 0's pointers (`seed` is not used)
};

// member p's seed and pieces of the scratch.  The kernels move the arrays they are passed themselves (mlp_rows_or_null).  (A copy of the pointers alone: a copy of the
// whole handle, whose offset tables the kernels index by the critic, would live in scratch memory.)
DI SacScratch sac_member(const SacDev& h, int p) {
  const size_t i = (size_t)p, B = (size_t)h.B, A = (size_t)h.A, n = (size_t)h.n_params, tiles = (size_t)h.tiles;
  SacScratch m = h.all;
  m.seed = h.seeds[p];
  m.a_pi += i * B * A;
  m.logp += i * B;
  m.logp_next += i * B;
  m.y += i * B;
  m.q += i * SAC_NQ * B;
  m.dqda += i * 2 * B * A;
  m.part += i * tiles * n;
  m.grad += i * n;
  m.loss_part += i * tiles * SAC_NLOSS;
  m.losses += i * 4;
  return m;
}

// [UPSTREAM] SquashedDiagGaussianDistribution: s.D [.][0 .. A) = mu, [A .. 2A) = the log_std head (kept: the clamp's gradient reads it); s.eps -> s.act = tanh(u),
// s.std = exp(clamp(log_std, -20, 2)), s.row[0] = logp, in double and rounded once.  One thread per row, components ascending.  The caller places the barriers.
DI void sac_squash(MlpLds& s, int A) {
  for (int r = (int)threadIdx.x; r < MLP_T; r += (int)blockDim.x) {
    double gauss = 0.0, corr = 0.0;
    for (int j = 0; j < A; j++) {
      const double mu = (double)s.D[r * MLP_DLD + j], ls = (double)fminf(fmaxf(s.D[r * MLP_DLD + A + j], -20.0f), 2.0f), e = (double)s.eps[r * 8 + j];
      const double sd = exp(ls), a = (double)(float)tanh(mu + sd * e);   // the action is the float32 value the critics read
      s.std[r * 8 + j] = (float)sd;
      s.act[r * 8 + j] = (float)a;
      gauss += -0.5 * e * e - ls - MLP_HALF_LOG_2PI;
      corr += log(1.0 - a * a + 1e-6);
    }
    s.row[0][r] = (float)(gauss - corr);
  }
}

DI float sac_alpha(const SacDev& h, const SacHyper& hy, const float* __restrict__ P) { return hy.auto_alpha ? expf(P[h.n_params - 1]) : hy.alpha_fixed; }

// ---- 1: the actor on obs (blockIdx.y = 0); the actor on next_obs and the targets (blockIdx.y = 1)
__global__ __launch_bounds__(MLP_BLOCK) void hrg_sac_policy_kernel(const SacDev h, const float* __restrict__ P, const float* __restrict__ PT, const float* __restrict__ obs,
                                                                   const float* __restrict__ nobs, const float* __restrict__ dones, const float* __restrict__ rewards,
                                                                   const float* __restrict__ eps_pi, const float* __restrict__ eps_next, uint64_t count) {
  __shared__ MlpLds s;
  const int row0 = (int)blockIdx.x * MLP_T, next = (int)blockIdx.y, p = (int)blockIdx.z, K = h.K, A = h.A;
  if (row0 >= h.B) return;   // (uniform over the workgroup)
  const SacScratch m = sac_member(h, p);
  const SacHyper hy = h.hyper[p];
  const size_t B = (size_t)h.B;
  P = mlp_rows_or_null(P, p, (size_t)h.n_params); PT = mlp_rows_or_null(PT, p, 2 * (size_t)h.n_critic);
  obs = mlp_rows_or_null(obs, p, B * K); nobs = mlp_rows_or_null(nobs, p, B * K); dones = mlp_rows_or_null(dones, p, B); rewards = mlp_rows_or_null(rewards, p, B);
  eps_pi = mlp_rows_or_null(eps_pi, p, B * A); eps_next = mlp_rows_or_null(eps_next, p, B * A);
  mlp_load(s, next ? nobs : obs, K, 0, row0, h.B);
  mlp_noise(s, next ? eps_next : eps_pi, A, row0, h.B, m.seed, count, STREAM_SAC, next ? HRG_ACT_DIM : 0);
  mlp_trunk(s, P, h.a_w, h.a_b, h.depth, K, MLP_ACT_RELU);
  mlp_head(s, P, h.a_hw, h.a_hb, h.depth, 2 * A);
  sac_squash(s, A);
  __syncthreads();
  const int t = (int)threadIdx.x;
  if (!next) {
    for (int i = t; i < MLP_T * A; i += (int)blockDim.x) m.a_pi[(size_t)(row0 + i / A) * A + i % A] = s.act[(i / A) * 8 + i % A];
    for (int r = t; r < MLP_T; r += (int)blockDim.x) m.logp[row0 + r] = s.row[0][r];
    return;
  }
  for (int r = t; r < MLP_T; r += (int)blockDim.x) s.row[3][r] = s.row[0][r];   // logp' (s.row[0] is each head's scratch no longer, but keep it apart)
  for (int i = t; i < MLP_T * A; i += (int)blockDim.x) s.X[(i / A) * MLP_XLD + K + i % A] = s.act[(i / A) * 8 + i % A];
  for (int c = 0; c < 2; c++) {
    const int32_t w[HRG_SAC_MAX_DEPTH] = {h.q_w[c][0] - h.n_actor, h.q_w[c][1] - h.n_actor, h.q_w[c][2] - h.n_actor};
    const int32_t b[HRG_SAC_MAX_DEPTH] = {h.q_b[c][0] - h.n_actor, h.q_b[c][1] - h.n_actor, h.q_b[c][2] - h.n_actor};
    mlp_trunk(s, PT, w, b, h.depth, K + A, MLP_ACT_RELU);
    mlp_head(s, PT, h.q_ow[c] - h.n_actor, h.q_ob[c] - h.n_actor, h.depth, 1);
    for (int r = t; r < MLP_T; r += (int)blockDim.x) s.row[1 + c][r] = s.D[r * MLP_DLD];
    __syncthreads();
  }
  const float alpha = sac_alpha(h, hy, P);
  for (int r = t; r < MLP_T; r += (int)blockDim.x) {
    const float q1 = s.row[1][r], q2 = s.row[2][r], lp = s.row[3][r];
    m.q[2 * h.B + row0 + r] = q1;
    m.q[3 * h.B + row0 + r] = q2;
    m.logp_next[row0 + r] = lp;
    m.y[row0 + r] = rewards[row0 + r] + (1.0f - dones[row0 + r]) * hy.gamma * (fminf(q1, q2) - alpha * lp);
  }
}

// ---- 2: critic blockIdx.y on (obs, act): forward, (q - y) / B, backward
__global__ __launch_bounds__(MLP_BLOCK) void hrg_sac_critic_kernel(const SacDev h, const float* __restrict__ P, const float* __restrict__ obs, const float* __restrict__ act) {
  __shared__ MlpLds s;
  const int row0 = (int)blockIdx.x * MLP_T, c = (int)blockIdx.y, p = (int)blockIdx.z, K = h.K, A = h.A, t = (int)threadIdx.x;
  if (row0 >= h.B) return;
  const SacScratch m = sac_member(h, p);
  P = mlp_rows_or_null(P, p, (size_t)h.n_params); obs = mlp_rows_or_null(obs, p, (size_t)h.B * K); act = mlp_rows_or_null(act, p, (size_t)h.B * A);
  mlp_load(s, obs, K, 0, row0, h.B);
  mlp_load(s, act, A, K, row0, h.B);
  mlp_trunk(s, P, h.q_w[c], h.q_b[c], h.depth, K + A, MLP_ACT_RELU);
  mlp_head(s, P, h.q_ow[c], h.q_ob[c], h.depth, 1);
  const float inv_b = 1.0f / (float)h.B;
  for (int r = t; r < MLP_T; r += (int)blockDim.x) {
    const float q = s.D[r * MLP_DLD], d = q - m.y[row0 + r];
    m.q[c * h.B + row0 + r] = q;
    s.row[0][r] = d * d;
    s.D[r * MLP_DLD] = d * inv_b;   // d (0.5 (mean (Q1 - y)^2 + mean (Q2 - y)^2)) / d q
  }
  __syncthreads();
  if (t == 0) {
    double sum = 0.0;
    for (int r = 0; r < MLP_T; r++) sum += (double)s.row[0][r];
    m.loss_part[blockIdx.x * SAC_NLOSS + c] = (float)sum;
  }
  mlp_backward(s, P, h.q_w[c], h.q_b[c], h.q_ow[c], h.q_ob[c], h.depth, K + A, 1, m.part + (size_t)blockIdx.x * h.n_params, true, 0, MLP_ACT_RELU);
}

// ---- 4: the updated critic blockIdx.y on (obs, a_pi): q and d q / d a
__global__ __launch_bounds__(MLP_BLOCK) void hrg_sac_actor_q_kernel(const SacDev h, const float* __restrict__ P, const float* __restrict__ obs) {
  __shared__ MlpLds s;
  const int row0 = (int)blockIdx.x * MLP_T, c = (int)blockIdx.y, p = (int)blockIdx.z, K = h.K, A = h.A, t = (int)threadIdx.x;
  if (row0 >= h.B) return;
  const SacScratch m = sac_member(h, p);
  P = mlp_rows_or_null(P, p, (size_t)h.n_params); obs = mlp_rows_or_null(obs, p, (size_t)h.B * K);
  mlp_load(s, obs, K, 0, row0, h.B);
  mlp_load(s, m.a_pi, A, K, row0, h.B);
  mlp_trunk(s, P, h.q_w[c], h.q_b[c], h.depth, K + A, MLP_ACT_RELU);
  mlp_head(s, P, h.q_ow[c], h.q_ob[c], h.depth, 1);
  for (int r = t; r < MLP_T; r += (int)blockDim.x) {
    m.q[(4 + c) * h.B + row0 + r] = s.D[r * MLP_DLD];
    s.D[r * MLP_DLD] = 1.0f;
  }
  __syncthreads();
  mlp_backward(s, P, h.q_w[c], h.q_b[c], h.q_ow[c], h.q_ob[c], h.depth, K + A, 1, nullptr, false, K + 1, MLP_ACT_RELU);
  for (int i = t; i < MLP_T * A; i += (int)blockDim.x) m.dqda[((size_t)c * h.B + row0 + i / A) * A + i % A] = s.D[(i / A) * MLP_DLD + i % A];
}

// ---- 5: the actor's loss mean(alpha logp - min(Q1, Q2)(obs, a_pi)) and its gradient
__global__ __launch_bounds__(MLP_BLOCK) void hrg_sac_actor_kernel(const SacDev h, const float* __restrict__ P, const float* __restrict__ obs, const float* __restrict__ eps_pi,
                                                                  uint64_t count) {
  __shared__ MlpLds s;
  const int row0 = (int)blockIdx.x * MLP_T, p = (int)blockIdx.z, K = h.K, A = h.A, t = (int)threadIdx.x;
  if (row0 >= h.B) return;
  const SacScratch m = sac_member(h, p);
  const SacHyper hy = h.hyper[p];
  P = mlp_rows_or_null(P, p, (size_t)h.n_params); obs = mlp_rows_or_null(obs, p, (size_t)h.B * K); eps_pi = mlp_rows_or_null(eps_pi, p, (size_t)h.B * A);
  mlp_load(s, obs, K, 0, row0, h.B);
  mlp_noise(s, eps_pi, A, row0, h.B, m.seed, count, STREAM_SAC, 0);
  mlp_trunk(s, P, h.a_w, h.a_b, h.depth, K, MLP_ACT_RELU);
  mlp_head(s, P, h.a_hw, h.a_hb, h.depth, 2 * A);
  sac_squash(s, A);
  __syncthreads();
  const float alpha = sac_alpha(h, hy, P), inv_b = 1.0f / (float)h.B;
  for (int r = t; r < MLP_T; r += (int)blockDim.x) {
    const float q1 = m.q[4 * h.B + row0 + r], q2 = m.q[5 * h.B + row0 + r];
    const float* dq = m.dqda + ((size_t)(q1 <= q2 ? 0 : 1) * h.B + row0 + r) * A;
    s.row[1][r] = alpha * s.row[0][r] - fminf(q1, q2);
    for (int j = 0; j < A; j++) {
      const float raw = s.D[r * MLP_DLD + A + j];
      const double a = (double)s.act[r * 8 + j], one = 1.0 - a * a;
      const double da = (double)alpha * (2.0 * a / (one + 1e-6)) - (double)dq[j];   // d / d a_j: logp's squash correction -log(1 - a^2 + 1e-6), and -Q
      const double du = da * one;                                                      // tanh
      const bool pass = raw >= -20.0f && raw <= 2.0f;                                  // the clamp passes a gradient inside its bounds only
      s.D[r * MLP_DLD + j] = (float)(du * (double)inv_b);                              // u = mu + std eps
      s.D[r * MLP_DLD + A + j] = pass ? (float)((du * (double)s.std[r * 8 + j] * (double)s.eps[r * 8 + j] - (double)alpha) * (double)inv_b) : 0.0f;   // ... and logp's own -log_std
    }
  }
  __syncthreads();
  if (t == 0) {
    double la = 0.0, lp = 0.0;
    for (int r = 0; r < MLP_T; r++) { la += (double)s.row[1][r]; lp += (double)s.row[0][r]; }
    m.loss_part[blockIdx.x * SAC_NLOSS + 2] = (float)la;
    m.loss_part[blockIdx.x * SAC_NLOSS + 3] = (float)lp;
  }
  mlp_backward(s, P, h.a_w, h.a_b, h.a_hw, h.a_hb, h.depth, K, 2 * A, m.part + (size_t)blockIdx.x * h.n_params, true, 0, MLP_ACT_RELU);
}

// ---- 3 and 6: parameters [lo, hi): the gradient (the tiles' parts in tile order), torch's Adam with eps 1e-8 (mlp_adam).  `target` non-null: target[i - lo] <-
// (1 - tau) target + tau param, the polyak update of the critics (lo = n_actor).  `coef` (the actor's launch): thread 0 of block 0 also sums the losses and, when
// the coefficient is learned, takes its gradient -mean(logp + target_entropy) and its Adam step.  Grid (blocks of [lo, hi), 1, members): the tail runs once per member.
// The learning rate and tau are the member's (SacHyper).
__global__ __launch_bounds__(MLP_BLOCK) void hrg_sac_adam_kernel(const SacDev h, float* __restrict__ P, float* __restrict__ M, float* __restrict__ V, int lo, int hi,
                                                                 double bc1, double bc2, float* __restrict__ target, int coef) {
  const int i = lo + (int)(blockIdx.x * blockDim.x + threadIdx.x), p = (int)blockIdx.z;
  const SacScratch m = sac_member(h, p);
  const SacHyper hy = h.hyper[p];
  const double lr = hy.lr, tau = hy.tau;
  P = mlp_rows_or_null(P, p, (size_t)h.n_params); M = mlp_rows_or_null(M, p, (size_t)h.n_params); V = mlp_rows_or_null(V, p, (size_t)h.n_params);
  target = mlp_rows_or_null(target, p, 2 * (size_t)h.n_critic);
  if (i < hi) {
    float g = m.part[i];
    for (int tl = 1; tl < h.tiles; tl++) g += m.part[(size_t)tl * h.n_params + i];
    m.grad[i] = g;
    const float p = mlp_adam(P, M, V, i, (double)g, lr, bc1, bc2, 1e-8);
    if (target) target[i - lo] = (float)((1.0 - tau) * (double)target[i - lo] + tau * (double)p);
  }
  if (coef && blockIdx.x == 0 && threadIdx.x == 0) {
    double sq1 = 0.0, sq2 = 0.0, la = 0.0, lp = 0.0;
    for (int tl = 0; tl < h.tiles; tl++) {
      sq1 += (double)m.loss_part[tl * SAC_NLOSS];
      sq2 += (double)m.loss_part[tl * SAC_NLOSS + 1];
      la += (double)m.loss_part[tl * SAC_NLOSS + 2];
      lp += (double)m.loss_part[tl * SAC_NLOSS + 3];
    }
    const double inv_b = 1.0 / (double)h.B;
    const int ia = h.n_params - 1;
    const float mean_lp = (float)(lp * inv_b + (double)hy.target_entropy);   // mean(logp + target_entropy)
    m.losses[0] = (float)(la * inv_b);
    m.losses[1] = (float)(0.5 * (sq1 + sq2) * inv_b);
    m.losses[2] = hy.auto_alpha ? -P[ia] * mean_lp : 0.0f;
    m.losses[3] = hy.auto_alpha ? expf(P[ia]) : hy.alpha_fixed;
    m.grad[ia] = 0.0f;
    if (hy.auto_alpha) {
      const float g = -mean_lp;
      m.grad[ia] = g;
      mlp_adam(P, M, V, ia, (double)g, lr, bc1, bc2, 1e-8);
    }
  }
}

// ---- the actor's forward pass on any number of rows: tanh(mu + std eps) or, deterministic, tanh(mu); a tile of rows per workgroup.  Grid (tiles of a group,
// members): obs, eps_in and out are [P][n][.], member blockIdx.y's actor on its group of n rows.  The tile's bound is the end of the group, and a draw's key
// the row's index in the group.
__global__ __launch_bounds__(MLP_BLOCK) void hrg_sac_act_kernel(const SacDev h, const float* __restrict__ P, const float* __restrict__ obs, int n, const float* __restrict__ eps_in,
                                                                int deterministic, uint64_t call, float* __restrict__ out) {
  __shared__ MlpLds s;
  const int row0 = (int)blockIdx.x * MLP_T, p = (int)blockIdx.y, K = h.K, A = h.A;
  if (row0 >= n) return;
  P = mlp_rows_or_null(P, p, (size_t)h.n_params); obs = mlp_rows_or_null(obs, p, (size_t)n * K); eps_in = mlp_rows_or_null(eps_in, p, (size_t)n * A); out = mlp_rows_or_null(out, p, (size_t)n * A);
  mlp_load(s, obs, K, 0, row0, n);
  if (deterministic) {
    for (int i = (int)threadIdx.x; i < MLP_T * 8; i += (int)blockDim.x) s.eps[i] = 0.0f;
  } else {
    mlp_noise(s, eps_in, A, row0, n, h.seeds[p], call, STREAM_SAC_ACT, 0);
  }
  mlp_trunk(s, P, h.a_w, h.a_b, h.depth, K, MLP_ACT_RELU);
  mlp_head(s, P, h.a_hw, h.a_hb, h.depth, 2 * A);
  sac_squash(s, A);
  __syncthreads();
  for (int i = (int)threadIdx.x; i < MLP_T * A; i += (int)blockDim.x)
    if (row0 + i / A < n) out[(size_t)(row0 + i / A) * A + i % A] = s.act[(i / A) * 8 + i % A];
}
