// hrgym_mlp.h -- what the device learners share (hrgym_sac.h, hrgym_ppo.h): the products of a multilayer perceptron of hidden width 64 and depth 1 .. 3 on a tile
// of rows, forward and backward, and Adam's update of one parameter.  Included into the base translation unit only (hrgym_hip.hip, HRG_BASE_TU), ahead of
// hrgym_sac.h.  No vendor BLAS, no autograd, no atomics, no waiting of one workgroup on another: a dependency is a launch boundary on one stream, and every loop has
// a bound known at launch.
//
// A tile is MLP_T = 32 rows of the batch (the batch is a multiple of 32), one workgroup of MLP_BLOCK = 256 threads, activations in LDS, the layer's weights staged
// into LDS before each product.  Plain FMA through LDS, float32 operands and double accumulators: a 32 x 64 x 64 product is 512 FMAs per thread.  The exact-f32 MFMA
// was not taken: it accumulates in float32, and with double accumulators the device sits below the float32 noise floor the tests measure instead of around it (the
// measured step time is in DESIGN.md D22 and profiles/r12_sac.json).
//
// Every sum has a fixed order that does not depend on the launch: a product sums k ascending with fma in a double accumulator (the float32 operands' products are
// exact there) and is rounded to float32 once, a weight gradient sums the tile's rows ascending and then the tiles ascending (in the learner's Adam or reduce
// kernel), a loss sums rows then tiles.  Two learners fed the same batches end bit-identical.
//
// The units are ReLU (SAC) or tanh (PPO); tanh is evaluated in double on the double accumulator and rounded once.  Adam's update is computed in double and rounded
// once into the float32 parameter.
#pragma once

#define MLP_T HRG_SAC_TILE   // rows per tile
#define MLP_BLOCK 256     // threads per workgroup
#define MLP_H HRG_SAC_HIDDEN
#define MLP_XLD 73        // row stride of the input tile (in0 <= 64 + 7 = 71; odd: lanes on consecutive rows meet distinct banks)
#define MLP_HLD 65        // ... of a hidden activation
#define MLP_WLD 72        // ... of the staged weights (read as broadcasts)
#define MLP_DLD 17        // ... of the heads' outputs (at most 14 columns)
#define MLP_HALF_LOG_2PI 0.91893853320467274178   // 0.5 log(2 pi), of the Gaussians' log densities

struct MlpLds {
  float X[MLP_T * MLP_XLD];
  float H[HRG_SAC_MAX_DEPTH][MLP_T * MLP_HLD];
  float W[MLP_H * MLP_WLD];
  float D[MLP_T * MLP_DLD];     // the heads' outputs, then their gradients
  float eps[MLP_T * 8], act[MLP_T * 8], std[MLP_T * 8];
  float row[4][MLP_T];          // per-row scalars
};

// ---- products on a tile.  Every thread of the workgroup calls them; the caller places the barriers.  `act` is a layer's activation, a constant at every call.  The
// tanh stores are loops of their own in front of the ReLU / linear ones, which stand as they stood before there was a parameter: in that form the SAC kernels
// compile to the instructions they had then.
enum { MLP_ACT_NONE = 0, MLP_ACT_RELU = 1, MLP_ACT_TANH = 2 };
// Ws[j][k] = Wg[j * in + k]
DI void mlp_stage(float* Ws, const float* __restrict__ Wg, int nout, int in) {
  for (int i = (int)threadIdx.x; i < nout * in; i += (int)blockDim.x) Ws[(i / in) * MLP_WLD + (i % in)] = Wg[i];
}

// out[r][j] = act(b[j] + sum_k X[r][k] Ws[j][k]), k ascending.  An item is a row and eight consecutive outputs.
DI void mlp_forward(const float* X, int ldx, int in, const float* Ws, const float* __restrict__ bg, int nout, int act, float* out, int ldo) {
  const int groups = (nout + 7) >> 3;
  for (int it = (int)threadIdx.x; it < MLP_T * groups; it += (int)blockDim.x) {
    const int r = it % MLP_T, j0 = (it / MLP_T) << 3, jn = min(8, nout - j0);
    double acc[8];
#pragma unroll
    for (int jj = 0; jj < 8; jj++) acc[jj] = jj < jn ? bg[j0 + jj] : 0.0f;
    for (int k = 0; k < in; k++) {
      const float x = X[r * ldx + k];
#pragma unroll
      for (int jj = 0; jj < 8; jj++)
        if (jj < jn) acc[jj] = fma((double)Ws[(j0 + jj) * MLP_WLD + k], (double)x, acc[jj]);
    }
    if (act == MLP_ACT_TANH) {
#pragma unroll
      for (int jj = 0; jj < 8; jj++)
        if (jj < jn) out[r * ldo + j0 + jj] = (float)tanh(acc[jj]);
      continue;
    }
    const bool relu = act == MLP_ACT_RELU;
#pragma unroll
    for (int jj = 0; jj < 8; jj++)
      if (jj < jn) out[r * ldo + j0 + jj] = relu ? fmaxf((float)acc[jj], 0.0f) : (float)acc[jj];
  }
}

// dst[r][k - k_lo] = sum_j dP[r][j] Ws[j][k] for k_lo <= k < in, j ascending; with an activation, dst holds the unit's output h the gradient passes through and
// becomes the gradient at its input (ReLU: 0 where the unit was off; tanh: times 1 - h^2).  An item is a row and eight consecutive k.
DI void mlp_backward_x(const float* dP, int ldp, int nout, const float* Ws, int in, int k_lo, float* dst, int ldd, int act) {
  const int groups = (in - k_lo + 7) >> 3;
  for (int it = (int)threadIdx.x; it < MLP_T * groups; it += (int)blockDim.x) {
    const int r = it % MLP_T, k0 = k_lo + ((it / MLP_T) << 3), kn = min(8, in - k0);
    double acc[8];
#pragma unroll
    for (int kk = 0; kk < 8; kk++) acc[kk] = 0.0f;
    for (int j = 0; j < nout; j++) {
      const float d = dP[r * ldp + j];
#pragma unroll
      for (int kk = 0; kk < 8; kk++)
        if (kk < kn) acc[kk] = fma((double)Ws[j * MLP_WLD + k0 + kk], (double)d, acc[kk]);
    }
    if (act == MLP_ACT_TANH) {
#pragma unroll
      for (int kk = 0; kk < 8; kk++)
        if (kk < kn) {
          float* p = dst + r * ldd + (k0 - k_lo) + kk;
          *p = (float)(acc[kk] * (1.0 - (double)*p * (double)*p));
        }
      continue;
    }
    const bool mask = act == MLP_ACT_RELU;
#pragma unroll
    for (int kk = 0; kk < 8; kk++)
      if (kk < kn) {
        float* p = dst + r * ldd + (k0 - k_lo) + kk;
        *p = (!mask || *p > 0.0f) ? (float)acc[kk] : 0.0f;
      }
  }
}

// gw[j * in + k] = sum_r dP[r][j] X[r][k], gb[j] = sum_r dP[r][j], r ascending over the tile's rows
DI void mlp_weight_grad(const float* dP, int ldp, int nout, const float* X, int ldx, int in, float* __restrict__ gw, float* __restrict__ gb) {
  for (int i = (int)threadIdx.x; i < nout * in; i += (int)blockDim.x) {
    const int j = i / in, k = i % in;
    double acc = 0.0;
    for (int r = 0; r < MLP_T; r++) acc = fma((double)dP[r * ldp + j], (double)X[r * ldx + k], acc);
    gw[i] = (float)acc;
  }
  for (int j = (int)threadIdx.x; j < nout; j += (int)blockDim.x) {
    double acc = 0.0;
    for (int r = 0; r < MLP_T; r++) acc += (double)dP[r * ldp + j];
    gb[j] = (float)acc;
  }
}

// the hidden layers: s.X [.][in0] -> s.H[0 .. depth - 1].  Ends with a barrier.
DI void mlp_trunk(MlpLds& s, const float* __restrict__ P, const int32_t* w, const int32_t* b, int depth, int in0, int act) {
  for (int l = 0; l < depth; l++) {
    const int in = l ? MLP_H : in0;
    __syncthreads();   // the input is written, the previous layer's weights are read
    mlp_stage(s.W, P + w[l], MLP_H, in);
    __syncthreads();
    mlp_forward(l ? s.H[l - 1] : s.X, l ? MLP_HLD : MLP_XLD, in, s.W, P + b[l], MLP_H, act, s.H[l], MLP_HLD);
  }
  __syncthreads();
}

// a linear head of `nout` outputs on s.H[depth - 1] -> s.D.  Ends with a barrier.
DI void mlp_head(MlpLds& s, const float* __restrict__ P, int w, int b, int depth, int nout) {
  mlp_stage(s.W, P + w, nout, MLP_H);   // (the trunk's barrier is behind the last read of s.W)
  __syncthreads();
  mlp_forward(s.H[depth - 1], MLP_HLD, MLP_H, s.W, P + b, nout, MLP_ACT_NONE, s.D, MLP_DLD);
  __syncthreads();
}

// the backward pass below a head whose gradient sits in s.D [.][nout]: the head's and every hidden layer's weight gradients into `g` (this tile's part), at the
// offsets of the parameters.  With `to_input` (0 or a first column k_lo + 1) the gradient at columns k_lo .. in0 - 1 of the input goes to s.D instead of the first
// layer's weight gradient being the end; `weights` = false skips every weight gradient (the actor's pass through a critic).  Ends with a barrier.
DI void mlp_backward(MlpLds& s, const float* __restrict__ P, const int32_t* w, const int32_t* b, int hw, int hb, int depth, int in0, int nout, float* g, bool weights,
                     int k_lo_plus1, int act) {
  if (weights) mlp_weight_grad(s.D, MLP_DLD, nout, s.H[depth - 1], MLP_HLD, MLP_H, g + hw, g + hb);
  mlp_stage(s.W, P + hw, nout, MLP_H);
  __syncthreads();
  mlp_backward_x(s.D, MLP_DLD, nout, s.W, MLP_H, 0, s.H[depth - 1], MLP_HLD, act);
  __syncthreads();
  for (int l = depth - 1; l >= 0; l--) {   // s.H[l] holds the gradient at layer l's pre-activation
    const int in = l ? MLP_H : in0;
    if (weights) mlp_weight_grad(s.H[l], MLP_HLD, MLP_H, l ? s.H[l - 1] : s.X, l ? MLP_HLD : MLP_XLD, in, g + w[l], g + b[l]);
    if (l == 0 && !k_lo_plus1) break;
    mlp_stage(s.W, P + w[l], MLP_H, in);
    __syncthreads();
    if (l) mlp_backward_x(s.H[l], MLP_HLD, MLP_H, s.W, MLP_H, 0, s.H[l - 1], MLP_HLD, act);
    else mlp_backward_x(s.H[0], MLP_HLD, MLP_H, s.W, in0, k_lo_plus1 - 1, s.D, MLP_DLD, MLP_ACT_NONE);
    __syncthreads();
  }
  __syncthreads();
}

// rows [row0, row0 + MLP_T) of src [n][width] into columns col0 .. of s.X; rows behind n become zero
DI void mlp_load(MlpLds& s, const float* __restrict__ src, int width, int col0, int row0, int n) {
  for (int i = (int)threadIdx.x; i < MLP_T * width; i += (int)blockDim.x) {
    const int r = i / width, c = i % width;
    s.X[r * MLP_XLD + col0 + c] = row0 + r < n ? src[(size_t)(row0 + r) * width + c] : 0.0f;
  }
}

// the noise of the tile's rows: supplied, or drawn
DI void mlp_noise(MlpLds& s, const float* __restrict__ eps_in, int A, int row0, int n, uint64_t seed, uint64_t count, uint64_t stream, int comp0) {
  for (int i = (int)threadIdx.x; i < MLP_T * A; i += (int)blockDim.x) {
    const int r = i / A, j = i % A;
    float e = 0.0f;
    if (row0 + r < n) e = eps_in ? eps_in[(size_t)(row0 + r) * A + j] : (float)rng_gauss(seed, count, (uint64_t)(row0 + r), stream, (uint64_t)(comp0 + j));
    s.eps[r * 8 + j] = e;
  }
}

// member p's part of an array of `stride` values per member (a population: hrgym_sac.h, hrgym_ppo.h).  mlp_rows_or_null: of an array that may be absent, null
// stays null -- at the price of a select, behind which the compiler no longer sees that the pointer is the kernel's read-only argument and loads what is uniform
// over the wave through the vector path; mlp_rows is for the arrays that are always there.
template <class T> DI T* mlp_rows(T* x, int p, size_t stride) { return x + (size_t)p * stride; }
template <class T> DI T* mlp_rows_or_null(T* x, int p, size_t stride) { return x ? x + (size_t)p * stride : x; }

// torch's Adam on parameter i with the gradient g (betas 0.9, 0.999, no weight decay; bias corrections bc1, bc2 = 1 - beta^t from the host), in double, rounded
// once into the float32 parameter, which it returns
DI float mlp_adam(float* __restrict__ P, float* __restrict__ M, float* __restrict__ V, int i, double g, double lr, double bc1, double bc2, double eps) {
  const double m = 0.9 * (double)M[i] + 0.1 * g, v = 0.999 * (double)V[i] + 0.001 * g * g;
  const float p = (float)((double)P[i] - lr * (m / bc1) / (sqrt(v / bc2) + eps));
  M[i] = (float)m;
  V[i] = (float)v;
  P[i] = p;
  return p;
}

// The rows of a population's hyper-parameter table (hrgym_sac.h: SacHyper, hrgym_ppo.h: PpoHyper) written from the launch's arguments, so that the upload is one
// more launch on the learner's stream: behind the steps queued there, ahead of the next, with no host memory the device reads later.  table[first + i] = c.rows[i]
// for i < count, or c.rows[0] in every one of them (`same`: the lone learner and the population whose members share their values).  One thread per row.
#define MLP_HYPER_CHUNK 16
template <class Row> struct MlpHyperChunk {
  Row rows[MLP_HYPER_CHUNK];
};
template <class Row> __global__ __launch_bounds__(64) void hrg_hyper_rows_kernel(Row* __restrict__ table, int first, int count, const MlpHyperChunk<Row> c, int same) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < count) table[first + i] = c.rows[same ? 0 : i % MLP_HYPER_CHUNK];
}
