// hrgym_dagger.h -- one DAgger step on the device (Ross, Gordon, Bagnell 2011): the states the learner's own policy reaches, labelled by the live scripted expert, as
// rows of a table that hrgym_bc.h's kernels train on.  Included into the base translation unit only (hrgym_hip.hip, HRG_BASE_TU), after hrgym_bc.h.  No LDS, no
// atomics; the grid is hrgym_buffer.h's: one wavefront per env, four per block.
//
// One launch per env step (hrg_dagger_step), between the learner's action and the step kernel:
//   hrg_dagger_step_kernel   env e: the label from the expert's row; the draw of who drives this step; the (view, label) pair into the table's row of the slot; the row the
//                            step kernel executes; the action the replay buffer keeps; the env's statistics.
//
// The label.  c = clip(expert_act[e][j], low[j], high[j]) in double.  SAC: 2 ((c - low) / (high - low)) - 1 in double, rounded to float32 once -- the value
// bc.demonstration_actions(scale = True) computes; the translation unit is compiled with -fapprox-func, so the division is the reciprocal refinement, within an ulp of
// the quotient in double, and the float32 label differs from numpy's only where the exact value sits next to a rounding boundary.  PPO: (float)c.
//
// The draw.  The expert drives env e this step iff rng_u01(seed, call, env_id0 + e, STREAM_DAGGER, 0) < beta: per step, independent of the sharding; beta = 0 never
// (u >= 0), beta = 1 always (u < 1).
//
// The executed row, double [HRG_ACT_DIM].  Expert: c.  Learner, SAC: low + 0.5 (a + 1) (high - low) in double, four rounded operations in torch's order
// (eval_unscale): what collect_steps sends.  Learner, PPO: the float32 action clamped by the float32 bounds, widened: what collect_rollout sends.  Zeros behind A.
//
// The table: [pinned + capacity_steps * n][K] and [..][A], the caller's memory; the row of step slot s, env e is pinned + s n + e.  The slot lives on the host.
//
// The statistics, double [n][HRG_DAGGER_STATS_DIM], lane j adds column j: steps, steps the expert drove, sum_j (a_j - label_j)^2 with a the learner's action at the
// label's scale (PPO: the clamped one), summed over j ascending.  Env e is touched by its own wave alone.
#pragma once

enum { STREAM_DAGGER = 16 };   // after STREAM_BC = 15 (hrgym_bc.h)

// one hrg_dagger; passed to the kernel by value.  The bounds are per-lane lookups: device memory, not kernel arguments.
struct DaggerDev {
  int32_t sac = 0, n = 0, K = 0, A = 0, pinned = 0;
  int64_t env_id0 = 0;
  uint64_t seed = 0;
  const double* low = nullptr;    // [HRG_ACT_DIM]
  const double* high = nullptr;   // [HRG_ACT_DIM]
  double* stats = nullptr;        // [n][HRG_DAGGER_STATS_DIM]
};

// grid = ceil(n / 4) blocks of four wavefronts, an env each.  kept may be null.
__global__ __launch_bounds__(HRG_BUFFER_BLOCK) void hrg_dagger_step_kernel(const DaggerDev h, const float* __restrict__ view, const float* __restrict__ learner_act,
                                                                           const double* __restrict__ expert_act, double beta, uint64_t call, int64_t slot,
                                                                           float* __restrict__ table_obs, float* __restrict__ table_act, double* __restrict__ rows_out,
                                                                           float* __restrict__ kept) {
  const int lane = (int)(threadIdx.x & 63);
  const int e = buffer_wave_item();
  if (e >= h.n) return;   // (wave-uniform: the ragged last block)
  const int K = h.K, A = h.A;
  const size_t row = (size_t)h.pinned + (size_t)slot * (size_t)h.n + (size_t)e;
  if (lane < K) table_obs[row * (size_t)K + lane] = view[(size_t)e * K + lane];   // lane k moves value k: one coalesced row
  const bool expert = rng_u01(h.seed, call, (uint64_t)(h.env_id0 + (int64_t)e), STREAM_DAGGER, 0) < beta;   // (the same value on every lane)
  double sq = 0.0;
  if (lane < A) {
    const double lo = h.low[lane], hi = h.high[lane], x = expert_act[(size_t)e * HRG_ACT_DIM + lane];
    const double c = x < lo ? lo : x > hi ? hi : x;   // np.clip: a NaN passes
    const float own = learner_act[(size_t)e * A + lane];
    float label, at_label;   // the label; the learner's action at the label's scale
    double run;              // what the learner's action executes
    if (h.sac) {
      label = (float)(2.0 * ((c - lo) / (hi - lo)) - 1.0);
      at_label = own;
      run = eval_unscale((double)own, lo, hi);
    } else {
      label = (float)c;
      const float flo = (float)lo, fhi = (float)hi;
      at_label = own < flo ? flo : own > fhi ? fhi : own;   // torch.clamp in float32: a NaN passes
      run = (double)at_label;
    }
    table_act[row * (size_t)A + lane] = label;
    rows_out[(size_t)e * HRG_ACT_DIM + lane] = expert ? c : run;
    if (kept) kept[(size_t)e * A + lane] = expert ? label : own;
    const double d = (double)at_label - (double)label;
    sq = d * d;
  } else if (lane < HRG_ACT_DIM) {
    rows_out[(size_t)e * HRG_ACT_DIM + lane] = 0.0;
  }
  double err = 0.0;
  for (int j = 0; j < A; j++) err += __shfl(sq, j);   // every lane of the wave takes part; j ascending
  if (lane < HRG_DAGGER_STATS_DIM) h.stats[(size_t)e * HRG_DAGGER_STATS_DIM + lane] += lane == HRG_DAGGER_STEPS ? 1.0 : lane == HRG_DAGGER_EXPERT_STEPS ? (expert ? 1.0 : 0.0) : err;
}
