// What one workgroup of the training step's kernels does, as __device__ functions of its block coordinates, and the shape
// rules of the step.  nn_train.hip (one network per handle) and nn_train_group.hip (a sweep of networks per launch) both
// build their kernels from these, so a network's bytes are the same whichever of the two trains it: same tile functions,
// same summation orders, same slice rule.  The host side the two share (layout, uploads, dataset, events) is nn_train_host.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "tile_gemm.h"
#include "tile_gemm_tn.h"

namespace nnmpc {

// Rows of the stacked batch of Bp padded samples: two passes for the structured form (0), one for the unstructured forms.
__host__ __device__ inline int train_rows(int form, int Bp) { return form == 0 ? 2 * Bp : Bp; }
// The same under the tangent loss (structured form only).  Block 0 is pass 1, block 1 pass 2; blocks 2 .. 2 + D - 1 are the D
// tangent blocks of pass 1 (one per direction of a row) and, with the whole-input form, blocks 2 + D .. 2 + 2D - 1 those of
// pass 2.  D = 1, whole = 0 is the one-direction form in [dx, (duprev)]: 3 Bp rows.
__host__ __device__ inline int train_rows_tan(int form, int Bp, int tan, int D = 1, int whole = 0) {
  return tan ? (2 + (whole ? 2 : 1) * D) * Bp : train_rows(form, Bp);
}

// Row slices of the dW reduction over M = train_rows(form, Bp) rows for a layer with `tiles` output tiles: as many as keep tiles x slices
// within the device's CUs (num_cus: the device property, 256 on MI355X) (one workgroup each: a second round would cost a
// whole slice time), at least 512 rows per slice, whole 32-row chunks.  Depends on the shape alone (and on the override
// force > 0, read once at create), never on timing.  Integer arithmetic only: host and device agree.
__host__ __device__ inline int dw_slices_wanted(int force, int num_cus, int M, int tiles) {   // non-decreasing in M
  const int a = num_cus / tiles > 1 ? num_cus / tiles : 1, b = M / 512 > 1 ? M / 512 : 1;
  const int S = force > 0 ? force : (a < b ? a : b);
  const int c = S < M / KC ? S : M / KC;
  return c > 1 ? c : 1;
}
__host__ __device__ inline int dw_slices(int force, int num_cus, int M, int tiles, int* slice_rows) {
  const int chunks = M / KC, S = dw_slices_wanted(force, num_cus, M, tiles);
  const int per = (chunks + S - 1) / S;
  *slice_rows = per * KC;
  return (chunks + per - 1) / per;
}

// nn_assemble_k's row layout (nn_forward.hip) from an f32 dataset, row b of the batch = dataset row idx[b] (idx == nullptr:
// first + b), for b = b_first, b_first + b_step, ... < Bp.  Samples b >= B and the pad columns are zero.
__device__ __forceinline__ void train_gather_rows(float* __restrict__ in, int ldk, int Bp, int B, int nx, int nu,
                                                  int with_uprev, const float* __restrict__ x,
                                                  const float* __restrict__ uprev, const float* __restrict__ xs,
                                                  const float* __restrict__ us, const int* __restrict__ idx, int first,
                                                  int b_first, int b_step) {
  const int o2 = nx + (with_uprev ? nu : 0);               // first column of the xs block
  const int din = o2 + nx + nu;
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int b = b_first; b < Bp; b += b_step) {
    float* d1 = in + (size_t)b * ldk;
    float* d2 = in + (size_t)(Bp + b) * ldk;
    if (b >= B) {
      for (int k = tid; k < ldk; k += nt) { d1[k] = 0.f; d2[k] = 0.f; }
      continue;
    }
    const size_t row = idx ? (size_t)idx[b] : (size_t)first + b;
    const float* xa = x + row * nx;
    const float* xb = xs + row * nx;
    const float* ub = us + row * nu;
    for (int k = tid; k < nx; k += nt) {
      const float xv = xa[k], sv = xb[k];
      d1[k] = xv; d1[o2 + k] = sv;
      d2[k] = sv; d2[o2 + k] = sv;
    }
    for (int k = tid; k < nu; k += nt) {
      const float uv = ub[k];
      d1[o2 + nx + k] = uv; d2[o2 + nx + k] = uv;
      if (with_uprev) { d1[nx + k] = uprev[row * nu + k]; d2[nx + k] = uv; }
    }
    for (int k = din + tid; k < ldk; k += nt) { d1[k] = 0.f; d2[k] = 0.f; }
  }
}

// Head output o [2Bp][ldo] -> pred = us + (o1 - o2), the squared error of the 64 samples of block `blk` as one fp64 partial
// (lanes add their elements in index order, then a fixed LDS tree), and, with dz != nullptr, the head-output gradient
// +g on pass-1 rows, -g on pass-2 rows, g = gscale (pred - u), exactly zero on padding rows and pad columns.  256 threads.
__device__ __forceinline__ void train_output_block(float* __restrict__ dz, const float* __restrict__ o, int ldo, int Bp,
                                                   int B, int nu, const float* __restrict__ us,
                                                   const float* __restrict__ u, const int* __restrict__ idx, int first,
                                                   float gscale, double* __restrict__ partial, int blk) {
  __shared__ double red[256];
  const int b0 = blk * 64, tid = threadIdx.x;
  double acc = 0.0;
  for (int e = tid; e < 64 * ldo; e += 256) {
    const int b = b0 + e / ldo, c = e % ldo;
    float g = 0.f;
    if (b < B && c < nu) {
      const size_t row = idx ? (size_t)idx[b] : (size_t)first + b;
      const float pred = us[row * nu + c] + (o[(size_t)b * ldo + c] - o[(size_t)(Bp + b) * ldo + c]);
      const float d = pred - u[row * nu + c];
      acc += (double)d * (double)d;
      g = gscale * d;
    }
    if (dz) {
      dz[(size_t)b * ldo + c] = g;
      dz[(size_t)(Bp + b) * ldo + c] = 0.f - g;
    }
  }
  red[tid] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) partial[blk] = red[0];
}

// The unstructured form (u = MLP([x, (uprev), xs, us]), one pass, a bias on the head): nn_assemble1_k's row layout
// (nn_forward.hip), ONE row per sample, so M = Bp rows.  Samples b >= B and the pad columns are zero.
__device__ __forceinline__ void train_gather_rows1(float* __restrict__ in, int ldk, int Bp, int B, int nx, int nu,
                                                   int with_uprev, const float* __restrict__ x,
                                                   const float* __restrict__ uprev, const float* __restrict__ xs,
                                                   const float* __restrict__ us, const int* __restrict__ idx, int first,
                                                   int b_first, int b_step) {
  const int o2 = nx + (with_uprev ? nu : 0);               // first column of the xs block
  const int din = o2 + nx + nu;
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int b = b_first; b < Bp; b += b_step) {
    float* d1 = in + (size_t)b * ldk;
    if (b >= B) {
      for (int k = tid; k < ldk; k += nt) d1[k] = 0.f;
      continue;
    }
    const size_t row = idx ? (size_t)idx[b] : (size_t)first + b;
    const float* xa = x + row * nx;
    const float* xb = xs + row * nx;
    const float* ub = us + row * nu;
    for (int k = tid; k < nx; k += nt) { d1[k] = xa[k]; d1[o2 + k] = xb[k]; }
    for (int k = tid; k < nu; k += nt) {
      d1[o2 + nx + k] = ub[k];
      if (with_uprev) d1[nx + k] = uprev[row * nu + k];
    }
    for (int k = din + tid; k < ldk; k += nt) d1[k] = 0.f;
  }
}

// Head output o [Bp][ldo] of the unstructured form -> pred = o (the head's epilogue has added the bias and, head_relu,
// applied the ReLU), the squared error of the 64 samples of block `blk` as one fp64 partial in train_output_block's order,
// and, with dz != nullptr, the head's dZ = gscale (pred - u); under head_relu 0 where pred <= 0 (derivative 0 at 0, a NaN
// passes, as in train_nt_mask_tile).  Exactly zero on padding rows and pad columns.  256 threads.
__device__ __forceinline__ void train_output1_block(float* __restrict__ dz, const float* __restrict__ o, int ldo, int B,
                                                    int nu, int head_relu, const float* __restrict__ u,
                                                    const int* __restrict__ idx, int first, float gscale,
                                                    double* __restrict__ partial, int blk) {
  __shared__ double red[256];
  const int b0 = blk * 64, tid = threadIdx.x;
  double acc = 0.0;
  for (int e = tid; e < 64 * ldo; e += 256) {
    const int b = b0 + e / ldo, c = e % ldo;
    float g = 0.f;
    if (b < B && c < nu) {
      const size_t row = idx ? (size_t)idx[b] : (size_t)first + b;
      const float pred = o[(size_t)b * ldo + c];
      const float d = pred - u[row * nu + c];
      acc += (double)d * (double)d;
      g = (head_relu && pred <= 0.f) ? 0.f : gscale * d;
    }
    if (dz) dz[(size_t)b * ldo + c] = g;
  }
  red[tid] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) partial[blk] = red[0];
}

// One thread adds the workgroup partials in index order: loss = scale * sum; acc += w * loss (the epoch's running sum).
__device__ __forceinline__ void train_loss_finish(const double* __restrict__ partial, int np, double scale, double w,
                                                  double* __restrict__ loss, double* __restrict__ acc) {
  double s = 0.0;
  for (int i = 0; i < np; ++i) s += partial[i];
  const double l = s * scale;
  *loss = l;
  *acc += w * l;
}

// Forward tile (tm, tn) of C = act(A B' + bias): gemm_nt_f32_k's tile (gemm_kernels.h) and epilogue.
template <int NB, bool RELU, bool BIAS>
__device__ __forceinline__ void train_fwd_tile(float* __restrict__ C, size_t ldc, const float* __restrict__ A, size_t lda,
                                               const float* __restrict__ B, size_t ldb, int K,
                                               const float* __restrict__ bias, int tm, int tn, float* lds) {
  using Cf = TileCfg<NB>;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int m0 = tm * NB, n0 = tn * NB;
  f32x16 acc[Cf::MT][Cf::MT];
  zero_acc<NB>(acc);
  PlainOp a{A + (size_t)m0 * lda, lda};
  PlainOp b{B + (size_t)n0 * ldb, ldb};
  tile_gemm_nt<NB>(acc, a, b, K, lds, false);
#pragma unroll
  for (int mi = 0; mi < Cf::MT; ++mi)
#pragma unroll
    for (int mj = 0; mj < Cf::MT; ++mj)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wr * Cf::WT + mi * 32 + acc_row(r, lane);
        const int col = n0 + wc * Cf::WT + mj * 32 + acc_col(lane);
        float v = acc[mi][mj][r];
        if (BIAS) v += bias[col];
        if (RELU) v = relu_nan(v);
        C[(size_t)row * ldc + col] = v;
      }
}

// ---- the tangent loss (structured form):  L = mean (pred - u)^2 + w mean (J d - t)^2,  J d the tangent of pred along a
// direction d of the row, propagated forward through the same weights in a row block of its own.  A row has D directions.
//   partial input  d = [dx, (duprev)]:            a'_0 = [dx, (duprev), 0, 0],  a'_l = (a'_{l-1} W_l) * [a_l(pass 1) > 0],
//                                                 J d = a'_{L-1} W_L                                      (no bias anywhere)
//   whole input    d = [dx, (duprev), dxs, dus]:  a'_0 = [dx, (duprev), dxs, dus] with the masks of pass 1,
//                                                 a''_0 = [dxs, (dus), dxs, dus]  with the masks of pass 2,
//                                                 J d = dus + (a'_{L-1} W_L - a''_{L-1} W_L), in f32 in that order, as pred is.
// Both means run over B D nu.  ReLU has no second derivative, so the masks are constants of the backward pass: the tangent
// rows are ordinary rows of dW = dZ' A, send nothing into the primal rows or the biases, and take their dA mask from the
// primal row they belong to (pass 1 for blocks 2 .. 2 + D - 1, pass 2 for the D after them).

// The tangent blocks of the gather: row (2 + d) Bp + b = [dx, (duprev), 0, 0] of direction d of dataset row idx[b] (tdx is
// [n][D][nx], tdup [n][D][nu]); with the whole-input form [dx, (duprev), dxs, dus] and row (2 + D + d) Bp + b = [dxs, (dus),
// dxs, dus].  Zero for b >= B and in the pad columns.  Same row walk as train_gather_rows, whose two blocks the same kernel writes.
__device__ __forceinline__ void train_gather_tan_rows(float* __restrict__ in, int ldk, int Bp, int B, int nx, int nu,
                                                      int with_uprev, int D, int whole, const float* __restrict__ tdx,
                                                      const float* __restrict__ tdup, const float* __restrict__ tdxs,
                                                      const float* __restrict__ tdus, const int* __restrict__ idx,
                                                      int first, int b_first, int b_step) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int dd = nx + (with_uprev ? nu : 0);               // width of [dx, (duprev)] = first column of the xs block
  const int din = dd + nx + nu;
  for (int b = b_first; b < Bp; b += b_step) {
    const size_t row = b >= B ? 0 : idx ? (size_t)idx[b] : (size_t)first + b;
    for (int d = 0; d < D; ++d) {
      float* d3 = in + ((size_t)(2 + d) * Bp + b) * ldk;
      float* d4 = in + ((size_t)(2 + D + d) * Bp + b) * ldk;   // whole input only
      if (b >= B) {
        for (int k = tid; k < ldk; k += nt) d3[k] = 0.f;
        if (whole) for (int k = tid; k < ldk; k += nt) d4[k] = 0.f;
        continue;
      }
      const size_t rd = row * D + d;
      for (int k = tid; k < nx; k += nt) d3[k] = tdx[rd * nx + k];
      if (with_uprev)
        for (int k = tid; k < nu; k += nt) d3[nx + k] = tdup[rd * nu + k];
      if (!whole) {
        for (int k = dd + tid; k < ldk; k += nt) d3[k] = 0.f;
        continue;
      }
      for (int k = tid; k < nx; k += nt) {
        const float sv = tdxs[rd * nx + k];
        d3[dd + k] = sv; d4[k] = sv; d4[dd + k] = sv;
      }
      for (int k = tid; k < nu; k += nt) {
        const float uv = tdus[rd * nu + k];
        d3[dd + nx + k] = uv; d4[dd + nx + k] = uv;
        if (with_uprev) d4[nx + k] = uv;
      }
      for (int k = din + tid; k < ldk; k += nt) { d3[k] = 0.f; d4[k] = 0.f; }
    }
  }
}

// train_output_block over o with the tangent blocks: the primal squared error and +-g exactly as there, and beside them
// e' = J d - t of the row's D directions, added in the order d = 0 .. D - 1 behind the primal term of the same element: a
// second fp64 partial (same lane order, same LDS tree).  J d is the head's tangent row (2 + d) Bp + b, or with the whole-input
// form dus + (that row - row (2 + D + d) Bp + b).  dZ'_L = gw e' on the pass-1 tangent rows and -gw e' on the pass-2 ones,
// gw = 2 w / (B D nu); exactly zero on padding rows and pad columns.  t and tdus are [n][D][nu].  256 threads.
__device__ __forceinline__ void train_output_tan_block(float* __restrict__ dz, const float* __restrict__ o, int ldo, int Bp,
                                                       int B, int nu, int D, int whole, const float* __restrict__ us,
                                                       const float* __restrict__ u, const float* __restrict__ t,
                                                       const float* __restrict__ tdus, const int* __restrict__ idx,
                                                       int first, float gscale, float gw, double* __restrict__ partial,
                                                       double* __restrict__ partial_tan, int blk) {
  __shared__ double red[2][256];
  const int b0 = blk * 64, tid = threadIdx.x;
  double acc = 0.0, acct = 0.0;
  for (int e = tid; e < 64 * ldo; e += 256) {
    const int b = b0 + e / ldo, c = e % ldo;
    const bool live = b < B && c < nu;
    const size_t row = !live ? 0 : idx ? (size_t)idx[b] : (size_t)first + b;
    float g = 0.f;
    if (live) {
      const float pred = us[row * nu + c] + (o[(size_t)b * ldo + c] - o[(size_t)(Bp + b) * ldo + c]);
      const float d = pred - u[row * nu + c];
      acc += (double)d * (double)d;
      g = gscale * d;
    }
    if (dz) {
      dz[(size_t)b * ldo + c] = g;
      dz[(size_t)(Bp + b) * ldo + c] = 0.f - g;
    }
    for (int d = 0; d < D; ++d) {
      const size_t r1 = ((size_t)(2 + d) * Bp + b) * ldo + c, r2 = ((size_t)(2 + D + d) * Bp + b) * ldo + c;
      float gt = 0.f;
      if (live) {
        const size_t at = (row * D + d) * nu + c;
        float jd = o[r1];
        if (whole) jd = tdus[at] + (jd - o[r2]);
        const float dt = jd - t[at];
        acct += (double)dt * (double)dt;
        gt = gw * dt;
      }
      if (dz) {
        dz[r1] = gt;
        if (whole) dz[r2] = 0.f - gt;
      }
    }
  }
  red[0][tid] = acc; red[1][tid] = acct;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) { red[0][tid] += red[0][tid + s]; red[1][tid] += red[1][tid + s]; }
    __syncthreads();
  }
  if (tid == 0) { partial[blk] = red[0][0]; partial_tan[blk] = red[1][0]; }
}

// train_loss_finish with the second sum: loss[0] = L = mse + w tan_mse (in double), loss[1] = mse = scale * sum,
// loss[2] = tan_mse = scale_tan * tangent sum (scale_tan = scale / D); acc[0..2] += weight * each (the epoch's running sums).
__device__ __forceinline__ void train_loss_finish_tan(const double* __restrict__ partial, const double* __restrict__ partial_tan,
                                                      int np, double scale, double scale_tan, double weight, double w,
                                                      double* __restrict__ loss, double* __restrict__ acc) {
  double s = 0.0, st = 0.0;
  for (int i = 0; i < np; ++i) s += partial[i];
  for (int i = 0; i < np; ++i) st += partial_tan[i];
  const double mse = s * scale, tan = st * scale_tan, l = mse + w * tan;
  loss[0] = l; loss[1] = mse; loss[2] = tan;
  acc[0] += weight * l; acc[1] += weight * mse; acc[2] += weight * tan;
}

// Hidden-layer forward of primal row tile tm TOGETHER with its D tangent tiles (a fan).  First the primal tile, byte for byte
// train_fwd_tile<NB, true, true> (same loop, same epilogue, same store order); the sign pattern of what it stored stays in
// registers, one bit per accumulator entry (16 MT^2 bits per lane: 64 at NB = 128).  Then the same workgroup runs the same
// tile_gemm_nt loop once per direction d over the tangent rows t0 + d Bp + tm NB ... against the same weights and stores that
// tile without bias, zero where the primal activation is <= 0 (derivative 0 at 0, a NaN passes, as in train_nt_mask_tile).
// t0 = 2 Bp for a pass-1 tile; for a pass-2 tile (tm NB >= Bp, whole-input form) t0 = (1 + D) Bp, so its tangents sit D blocks
// further down.  One GEMM after the other: no LDS beyond the 4 stages and no accumulators beyond the one set, so two
// workgroups per CU still fit.
template <int NB>
__device__ __forceinline__ void train_fwd_fan_tile(float* __restrict__ C, size_t ldc, const float* __restrict__ A,
                                                   size_t lda, const float* __restrict__ B, size_t ldb, int K,
                                                   const float* __restrict__ bias, int Bp, int D, int t0, int tm, int tn,
                                                   float* lds) {
  using Cf = TileCfg<NB>;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int m0 = tm * NB, n0 = tn * NB;
  f32x16 acc[Cf::MT][Cf::MT];
  zero_acc<NB>(acc);
  PlainOp b{B + (size_t)n0 * ldb, ldb};
  {
    PlainOp a{A + (size_t)m0 * lda, lda};
    tile_gemm_nt<NB>(acc, a, b, K, lds, false);
  }
  uint32_t live[Cf::MT][Cf::MT];                            // bit r: entry r of acc[mi][mj] has a non-zero derivative
#pragma unroll
  for (int mi = 0; mi < Cf::MT; ++mi)
#pragma unroll
    for (int mj = 0; mj < Cf::MT; ++mj) {
      uint32_t bits = 0;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wr * Cf::WT + mi * 32 + acc_row(r, lane);
        const int col = n0 + wc * Cf::WT + mj * 32 + acc_col(lane);
        float v = acc[mi][mj][r];
        v += bias[col];
        v = relu_nan(v);
        C[(size_t)row * ldc + col] = v;
        bits |= (v <= 0.f ? 0u : 1u) << r;
      }
      live[mi][mj] = bits;
    }
  for (int d = 0; d < D; ++d) {
    const int tr0 = t0 + d * Bp + m0;                       // first row of tangent tile d
    zero_acc<NB>(acc);
    {
      PlainOp a{A + (size_t)tr0 * lda, lda};
      tile_gemm_nt<NB>(acc, a, b, K, lds, false);
    }
#pragma unroll
    for (int mi = 0; mi < Cf::MT; ++mi)
#pragma unroll
      for (int mj = 0; mj < Cf::MT; ++mj)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = tr0 + wr * Cf::WT + mi * 32 + acc_row(r, lane);
          const int col = n0 + wc * Cf::WT + mj * 32 + acc_col(lane);
          C[(size_t)row * ldc + col] = (live[mi][mj] >> r) & 1u ? acc[mi][mj][r] : 0.f;
        }
  }
}

// The one-direction pair in [dx, (duprev)]: the fan of pass-1 row tile tm at D = 1, t0 = 2 Bp, written out with its constants.
// Folding the constants into train_fwd_fan_tile leaves the compiler another schedule and register assignment; this text keeps
// the pair kernels' instruction stream what it was before the fan existed, so a one-direction handle and the grouped trainer
// run unchanged code.
template <int NB>
__device__ __forceinline__ void train_fwd_pair_tile(float* __restrict__ C, size_t ldc, const float* __restrict__ A,
                                                    size_t lda, const float* __restrict__ B, size_t ldb, int K,
                                                    const float* __restrict__ bias, int Bp, int tm, int tn, float* lds) {
  using Cf = TileCfg<NB>;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int m0 = tm * NB, n0 = tn * NB;
  f32x16 acc[Cf::MT][Cf::MT];
  zero_acc<NB>(acc);
  PlainOp b{B + (size_t)n0 * ldb, ldb};
  {
    PlainOp a{A + (size_t)m0 * lda, lda};
    tile_gemm_nt<NB>(acc, a, b, K, lds, false);
  }
  uint32_t live[Cf::MT][Cf::MT];                            // bit r: entry r of acc[mi][mj] has a non-zero derivative
#pragma unroll
  for (int mi = 0; mi < Cf::MT; ++mi)
#pragma unroll
    for (int mj = 0; mj < Cf::MT; ++mj) {
      uint32_t bits = 0;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wr * Cf::WT + mi * 32 + acc_row(r, lane);
        const int col = n0 + wc * Cf::WT + mj * 32 + acc_col(lane);
        float v = acc[mi][mj][r];
        v += bias[col];
        v = relu_nan(v);
        C[(size_t)row * ldc + col] = v;
        bits |= (v <= 0.f ? 0u : 1u) << r;
      }
      live[mi][mj] = bits;
    }
  zero_acc<NB>(acc);
  {
    PlainOp a{A + (size_t)(2 * Bp + m0) * lda, lda};
    tile_gemm_nt<NB>(acc, a, b, K, lds, false);
  }
#pragma unroll
  for (int mi = 0; mi < Cf::MT; ++mi)
#pragma unroll
    for (int mj = 0; mj < Cf::MT; ++mj)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 2 * Bp + m0 + wr * Cf::WT + mi * 32 + acc_row(r, lane);
        const int col = n0 + wc * Cf::WT + mj * 32 + acc_col(lane);
        C[(size_t)row * ldc + col] = (live[mi][mj] >> r) & 1u ? acc[mi][mj][r] : 0.f;
      }
}

// dW planes: P[z][m][n] = sum over the rows r of slice z of A[r][m] * B[r][n]  (A = dZ_l, B = A_{l-1}); tile (by, bx) of slice bz.
template <int NB>
__device__ __forceinline__ void train_tn_tile(float* __restrict__ P, size_t plane, size_t ldp, const float* __restrict__ A,
                                              size_t lda, const float* __restrict__ B, size_t ldb, int rows, int slice_rows,
                                              int bx, int by, int bz, float* lds) {
  using Cf = TileCfg<NB>;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int m0 = by * NB, n0 = bx * NB;
  const int r0 = bz * slice_rows, r1 = min(rows, r0 + slice_rows);
  f32x16 acc[Cf::MT][Cf::MT];
  zero_acc<NB>(acc);
  if (r1 > r0) tile_gemm_tn<NB>(acc, A + (size_t)r0 * lda + m0, lda, B + (size_t)r0 * ldb + n0, ldb, r1 - r0, lds);
  float* Pz = P + (size_t)bz * plane;
#pragma unroll
  for (int mi = 0; mi < Cf::MT; ++mi)
#pragma unroll
    for (int mj = 0; mj < Cf::MT; ++mj)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wr * Cf::WT + mi * 32 + acc_row(r, lane);
        const int col = n0 + wc * Cf::WT + mj * 32 + acc_col(lane);
        Pz[(size_t)row * ldp + col] = acc[mi][mj][r];
      }
}

// dZ_{l-1} = (dZ_l W_l) * relu'(A_{l-1}):  C = A B' with B = the [in][out] copy of W_l, masked in the epilogue by the
// activation tile of the layer below (same shape and stride as C).  The derivative at 0 is 0 (a NaN passes), as in torch.
template <int NB>
__device__ __forceinline__ void train_nt_mask_tile(float* __restrict__ C, size_t ldc, const float* __restrict__ A,
                                                   size_t lda, const float* __restrict__ B, size_t ldb, int K,
                                                   const float* __restrict__ act, int bx, int by, float* lds) {
  using Cf = TileCfg<NB>;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int m0 = by * NB, n0 = bx * NB;
  f32x16 acc[Cf::MT][Cf::MT];
  zero_acc<NB>(acc);
  PlainOp a{A + (size_t)m0 * lda, lda};
  PlainOp b{B + (size_t)n0 * ldb, ldb};
  tile_gemm_nt<NB>(acc, a, b, K, lds, false);
#pragma unroll
  for (int mi = 0; mi < Cf::MT; ++mi)
#pragma unroll
    for (int mj = 0; mj < Cf::MT; ++mj)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wr * Cf::WT + mi * 32 + acc_row(r, lane);
        const int col = n0 + wc * Cf::WT + mj * 32 + acc_col(lane);
        const size_t at = (size_t)row * ldc + col;
        C[at] = act[at] <= 0.f ? 0.f : acc[mi][mj][r];
      }
}

// Bias-gradient partials: P[s][c] = sum of dZ[r][c] over the 128 rows of block s = by.  Thread (c, q) adds rows q, q+4, ...
// in order, then the four q are added in order.  64 columns per block bx, 256 threads.
__device__ __forceinline__ void train_colsum_block(float* __restrict__ P, const float* __restrict__ dz, int ld, int bx, int by) {
  __shared__ float red[4][64];
  const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int col = bx * 64 + c;
  const float* p = dz + (size_t)by * 128 * ld + col;
  float s = 0.f;
  for (int r = q; r < 128; r += 4) s += p[(size_t)r * ld];
  red[q][c] = s;
  __syncthreads();
  if (q == 0) P[(size_t)by * ld + col] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}

// THE gradient of an entry: its partial planes added in plane order.  train_adam_* and train_plane_sum_k (what
// nnmpc_train_grad returns) both call it, so the gradient a step applies is the one grad reports, bit for bit.
__device__ __forceinline__ float plane_sum(const float* __restrict__ P, size_t plane, int S, size_t at) {
  float g = P[at];
  for (int s = 1; s < S; ++s) g += P[(size_t)s * plane + at];
  return g;
}

struct AdamCoef { double omb1, b2, omb2, step, bc2s, eps; };   // 1 - beta1, beta2, 1 - beta2, lr / (1 - beta1^t), sqrt(1 - beta2^t), eps

// The scalars of Adam step t (t >= 1), in double on the host.
inline AdamCoef adam_coef(double lr, double beta1, double beta2, double eps, long t) {
  AdamCoef k;
  k.omb1 = 1.0 - beta1; k.b2 = beta2; k.omb2 = 1.0 - beta2;
  k.step = lr / (1.0 - pow(beta1, (double)t));
  k.bc2s = sqrt(1.0 - pow(beta2, (double)t));
  k.eps = eps;
  return k;
}

// torch.optim.Adam's update of one entry: m, v, w are f32 in memory, the arithmetic in between is fp64 (about two
// million entries per step at the widest network: not measurable), so an entry carries the rounding of its three stores only.
__device__ __forceinline__ float adam_entry(float g, float* m, float* v, float w, const AdamCoef& k) {
  const double gd = g;
  const double mn = (double)*m + (gd - (double)*m) * k.omb1;
  const double vn = k.b2 * (double)*v + k.omb2 * gd * gd;
  *m = (float)mn; *v = (float)vn;
  return (float)((double)w - k.step * (mn / (sqrt(vn) / k.bc2s + k.eps)));
}

// One 64 x 64 tile (bx: in, by: out) of W per workgroup: Wt [out][in] (the forward's operand) is updated in place and the
// same values go, through an LDS transpose, to Wk [in][out] (the dA GEMM's operand) -- no transpose pass.  256 threads.
__device__ __forceinline__ void train_adam_w_tile(float* __restrict__ Wt, float* __restrict__ Wk, float* __restrict__ m,
                                                  float* __restrict__ v, const float* __restrict__ P, size_t plane, int S,
                                                  int kpad, int npad, const AdamCoef& k, int bx, int by) {
  __shared__ float t[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int i0 = bx * 64, o0 = by * 64;
#pragma unroll 4
  for (int j = 0; j < 16; ++j) {
    const int ol = ty + 4 * j;
    const size_t at = (size_t)(o0 + ol) * kpad + i0 + tx;
    const float w = adam_entry(plane_sum(P, plane, S, at), m + at, v + at, Wt[at], k);
    Wt[at] = w;
    t[ol][tx] = w;
  }
  __syncthreads();
#pragma unroll 4
  for (int j = 0; j < 16; ++j) {
    const int il = ty + 4 * j;
    Wk[(size_t)(i0 + il) * npad + o0 + tx] = t[tx][il];
  }
}

}  // namespace nnmpc
