// TN tile GEMM core for gfx950:  acc[m][n] += sum_k A[k][m] * B[k][n]
// (both operands row-major with the REDUCTION index k as the slow one -- the weight gradient dW = dZ' A of a dense
// layer, k = the batch row), exact-f32 MFMA (v_mfma_f32_32x32x2_f32), 256 threads = 4 wave64 per NB x NB output tile.
// Accumulator map, wave grid and double buffering are tile_gemm.h's.
//
// LDS image per operand and K-chunk: [KC=32 k][NB floats], no padding.  A chunk row is NB consecutive floats of one
// global row, so staging is float4 loads and stores; a fragment read is one ds_read_b32 per MFMA step with lane l&31
// over m, i.e. 32 consecutive dwords per half wave (ds_read_b32 banks by 32 within each 32-lane half: conflict-free),
// and the two halves read the rows k = s and k = 16 + s of the chunk, tile_gemm.h's k map.
#pragma once
#include "tile_gemm.h"

namespace nnmpc {

template <int NB>
struct TileCfgTN {
  static constexpr int LD4 = KC * (NB / 4) / 256;      // float4 loads / thread / operand / chunk
  static constexpr int STAGE_FLOATS = KC * NB;         // one operand, one buffer
  static constexpr int LDS_FLOATS = 4 * STAGE_FLOATS;  // A,B x double buffer
};

// Global -> registers for one operand chunk: k rows [0,32) x columns [0,NB); `g` points at (k = k0, column 0 of the tile).
template <int NB>
__device__ __forceinline__ void load_chunk_tn(f32x4 (&r)[TileCfgTN<NB>::LD4], const float* __restrict__ g, size_t ld,
                                              int tid) {
#pragma unroll
  for (int i = 0; i < TileCfgTN<NB>::LD4; ++i) {
    const int f = tid + 256 * i;
    const int k = f / (NB / 4), c4 = f % (NB / 4);
    r[i] = *reinterpret_cast<const f32x4*>(g + (size_t)k * ld + 4 * c4);
  }
}
template <int NB>
__device__ __forceinline__ void store_chunk_tn(const f32x4 (&r)[TileCfgTN<NB>::LD4], float* s, int tid) {
#pragma unroll
  for (int i = 0; i < TileCfgTN<NB>::LD4; ++i) {
    const int f = tid + 256 * i;
    const int k = f / (NB / 4), c4 = f % (NB / 4);
    *reinterpret_cast<f32x4*>(s + k * NB + 4 * c4) = r[i];
  }
}

// One staged chunk (already in LDS): acc += A_chunk' * B_chunk.
template <int NB>
__device__ __forceinline__ void mma_chunk_tn(f32x16 (&acc)[TileCfg<NB>::MT][TileCfg<NB>::MT],
                                             const float* __restrict__ sA, const float* __restrict__ sB, int wr, int wc,
                                             int lane) {
  constexpr int MT = TileCfg<NB>::MT;
  constexpr int WT = TileCfg<NB>::WT;
  const int lr = lane & 31, kh = (lane >> 5) * 16;
  float a[MT][16], b[MT][16];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      a[m][s] = sA[(kh + s) * NB + wr * WT + m * 32 + lr];
      b[m][s] = sB[(kh + s) * NB + wc * WT + m * 32 + lr];
    }
#pragma unroll
  for (int s = 0; s < 16; ++s)
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int mj = 0; mj < MT; ++mj)
        acc[mi][mj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi][s], b[mj][s], acc[mi][mj], 0, 0, 0);
}

// acc += A[0:K, 0:NB]' * B[0:K, 0:NB]   (K multiple of 32; A, B point at (k = 0, first column of the tile)).
// All 256 threads; one barrier per chunk, as tile_gemm_nt.
template <int NB>
__device__ __forceinline__ void tile_gemm_tn(f32x16 (&acc)[TileCfg<NB>::MT][TileCfg<NB>::MT],
                                             const float* __restrict__ A, size_t lda, const float* __restrict__ B,
                                             size_t ldb, int K, float* lds) {
  using C = TileCfgTN<NB>;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int nk = K / KC;
  if (nk == 0) return;
  f32x4 ra[C::LD4], rb[C::LD4];
  load_chunk_tn<NB>(ra, A, lda, tid);
  load_chunk_tn<NB>(rb, B, ldb, tid);
  for (int kc = 0; kc < nk; ++kc) {
    float* sA = lds + (kc & 1) * 2 * C::STAGE_FLOATS;
    float* sB = sA + C::STAGE_FLOATS;
    store_chunk_tn<NB>(ra, sA, tid);
    store_chunk_tn<NB>(rb, sB, tid);
    __syncthreads();
    if (kc + 1 < nk) {
      load_chunk_tn<NB>(ra, A + (size_t)(kc + 1) * KC * lda, lda, tid);
      load_chunk_tn<NB>(rb, B + (size_t)(kc + 1) * KC * ldb, ldb, tid);
    }
    mma_chunk_tn<NB>(acc, sA, sB, wr, wc, lane);
  }
  __syncthreads();
}

}  // namespace nnmpc
