// hrgym_bc.h -- one behaviour-cloning step on the device: supervised pre-training of a learner's actor on a table of (observation, expert action) rows, the
// use SB2's `pretrain` made of a demonstration set for Box actions.  Included into the base translation unit only (hrgym_hip.hip, HRG_BASE_TU), after
// hrgym_ppo.h and hrgym_eval.h: the networks are hrgym_mlp.h's tile products, and its rules hold here (no vendor BLAS, no autograd, no atomics, a fixed order of
// every sum); the actor is named by EvalActor, the offsets of the learner's own handle (SacDev / PpoDev) -- the layout is not restated.
//
// One step is two launches (hrg_bc_step):
//   1 hrg_bc_grad_kernel  grid (tiles of 32 rows): the tile's table indices, drawn or supplied; the observation and action rows gathered straight from the table
//                         (no sample launch, no batch copy); the actor's trunk and mean head forward; the loss and its gradient at the head's outputs; backward
//                         -> this tile's part of the gradient and of the loss sum.
//   2 hrg_bc_adam_kernel  the entries the loss reaches: the tiles' parts summed in tile order, torch's Adam with eps 1e-8 (mlp_adam) on moments and a step count
//                         that belong to the bc handle; thread 0 of block 0 sums the loss.
//
// The loss is the mean squared error on the deterministic action, averaged over rows and components: SAC mean((tanh(mu(obs)) - a)^2), the squash in double per
// component and rounded once into the float32 action (as sac_squash), its derivative 1 - a^2 from that value; PPO mean((mu(obs) - a)^2).  Not the squashed
// Gaussian's likelihood: gripper commands sit at exactly +-1, where atanh is infinite.
//
// The loss reaches the hidden layers and the mean head alone -- three ranges of the parameter vector (BcDev.lo / n): the trunk, the head's first A weight rows,
// its first A biases.  SAC: actor.latent_pi.*, actor.mu.* (the log_std head's rows lie behind mu's in the [2A][64] product and are not read).  PPO: network 0 (the
// shared trunk, or mlp_extractor.policy_net) and action_net.* (value_net's row lies behind action_net's in the [A + 1][64] product).  No other entry of the
// parameters, and nothing of the learner's moments or counters, is written.
//
// Draws: row k of the batch takes table row min(floor(u n_rows), n_rows - 1), u = rng_u01 keyed by (bc seed, bc step count, k, STREAM_BC, 0): independent of the
// grid.  A supplied index is clamped into the table (the Python side raises IndexError before the launch).
#pragma once

enum { STREAM_BC = 15 };   // after STREAM_PPO_ACT = 14 (hrgym_ppo.h)
#define BC_NRANGE 3

// one hrg_bc: the learner's actor, the ranges the loss reaches, the scratch the handle owns; passed to the kernels by value
struct BcDev {
  EvalActor a;                      // hidden layers, the mean head (nout = A), depth, K, A, n_params
  int32_t sac = 0, B = 0, tiles = 0, n_reach = 0;
  int32_t lo[BC_NRANGE] = {0}, n[BC_NRANGE] = {0};   // trunk | the head's weights | its biases: first entry, entries
  uint64_t seed = 0;
  int64_t* index = nullptr;         // [B] the last step's table rows
  float* pred = nullptr;            // [B][A] the actor's deterministic actions
  float* part = nullptr;            // [tiles][n_params] the tiles' parts of the gradient (written in the three ranges only)
  float* grad = nullptr;            // [n_params] their sum; zero where the loss does not reach
  float* loss_part = nullptr;       // [tiles] sum over the tile's rows and components of the squared error
  float* loss = nullptr;            // [1]
};

// the i-th entry the loss reaches -> its offset in the parameter vector; -1 behind the last
DI int bc_entry(const BcDev& h, int i) {
  for (int k = 0; k < BC_NRANGE; k++) {
    if (i < h.n[k]) return h.lo[k] + i;
    i -= h.n[k];
  }
  return -1;
}

// ---- 1: the tile's rows of the table, forward, the loss, backward
__global__ __launch_bounds__(MLP_BLOCK) void hrg_bc_grad_kernel(const BcDev h, const float* __restrict__ P, const float* __restrict__ table_obs,
                                                                const float* __restrict__ table_act, int64_t n_rows, const int64_t* __restrict__ index_in,
                                                                uint64_t count) {
  __shared__ MlpLds s;
  __shared__ int64_t rows[MLP_T];
  const int row0 = (int)blockIdx.x * MLP_T, K = h.a.K, A = h.a.A, t = (int)threadIdx.x;
  if (row0 >= h.B) return;   // (uniform over the workgroup)
  const int unit = h.sac ? MLP_ACT_RELU : MLP_ACT_TANH;
  if (t < MLP_T) {
    const int k = row0 + t;
    int64_t i = index_in ? index_in[k] : (int64_t)floor(rng_u01(h.seed, count, (uint64_t)k, STREAM_BC, 0) * (double)n_rows);
    i = min(max(i, (int64_t)0), n_rows - 1);   // (u < 1: the bound keeps a draw inside the table whatever the rounding)
    rows[t] = i;
    h.index[k] = i;
  }
  __syncthreads();
  for (int i = t; i < MLP_T * K; i += (int)blockDim.x) s.X[(i / K) * MLP_XLD + i % K] = table_obs[(size_t)rows[i / K] * K + i % K];
  for (int i = t; i < MLP_T * A; i += (int)blockDim.x) s.act[(i / A) * 8 + i % A] = table_act[(size_t)rows[i / A] * A + i % A];
  mlp_trunk(s, P, h.a.w, h.a.b, h.a.depth, K, unit);
  mlp_head(s, P, h.a.hw, h.a.hb, h.a.depth, A);
  const double scale = 2.0 / ((double)h.B * (double)A);   // d mean(e^2) / d e
  for (int r = t; r < MLP_T; r += (int)blockDim.x) {
    double sq = 0.0;
    for (int j = 0; j < A; j++) {
      const float mu = s.D[r * MLP_DLD + j], a = h.sac ? (float)tanh((double)mu) : mu;   // the action is the float32 value the learner's act emits
      const double e = (double)a - (double)s.act[r * 8 + j], da = h.sac ? 1.0 - (double)a * (double)a : 1.0;
      sq += e * e;
      h.pred[(size_t)(row0 + r) * A + j] = a;
      s.D[r * MLP_DLD + j] = (float)(scale * e * da);
    }
    s.row[0][r] = (float)sq;
  }
  __syncthreads();
  if (t == 0) {
    double sum = 0.0;
    for (int r = 0; r < MLP_T; r++) sum += (double)s.row[0][r];
    h.loss_part[blockIdx.x] = (float)sum;
  }
  mlp_backward(s, P, h.a.w, h.a.b, h.a.hw, h.a.hb, h.a.depth, K, A, h.part + (size_t)blockIdx.x * h.a.n_params, true, 0, unit);
}

// ---- 2: entry i of the ones the loss reaches: the gradient (the tiles' parts in tile order, in double, rounded once), torch's Adam with eps 1e-8 on the bc
// handle's moments; thread 0 of block 0: the loss.  Grid = blocks of 256 over n_reach.
__global__ __launch_bounds__(MLP_BLOCK) void hrg_bc_adam_kernel(const BcDev h, float* __restrict__ P, float* __restrict__ M, float* __restrict__ V, double lr, double bc1,
                                                                double bc2) {
  const int e = bc_entry(h, (int)(blockIdx.x * blockDim.x + threadIdx.x));
  if (e >= 0) {
    double sum = 0.0;
    for (int tl = 0; tl < h.tiles; tl++) sum += (double)h.part[(size_t)tl * h.a.n_params + e];
    const float g = (float)sum;
    h.grad[e] = g;
    mlp_adam(P, M, V, e, (double)g, lr, bc1, bc2, 1e-8);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double sum = 0.0;
    for (int tl = 0; tl < h.tiles; tl++) sum += (double)h.loss_part[tl];
    h.loss[0] = (float)(sum / ((double)h.B * (double)h.a.A));
  }
}
