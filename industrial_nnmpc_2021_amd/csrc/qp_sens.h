// Directional derivatives of the box-QP solution restricted to the delivered active set (gfx950), nnmpc_qp_sensitivity.
//
// With the active set A (and its sides) fixed, u* is affine in (x0, lb, ub).  For a direction (dx0, dlb, dub):
//     du_i = dub_c | dlb_c  on A (i = k nu + c; copied),        t = Kunc dx0,   lam = (Hinv_AA)^-1 (t_A - du_A),   du = t - Hinv[:, A] lam
// so that P du + tq dx0 = 0 on the free rows and = -lam on the active ones (Hinv = P^-1, Kunc = -Hinv tq, both fp64 on the handle).
//
// sens_k: one workgroup of four waves per problem; all D directions of the problem share ONE factorisation.
//   1. the ordered list of the active variables and their sides from the words: trips of 256 variables, wave ballots, no atomics
//      (as asm_mult_k does); m = |A|, counted beyond what the list holds;
//   2. the flag, before anything is stored: 2 = no answer (status NNMPC_ST_NUMERIC, both bits of one variable, a non-finite
//      perturbation in any of the problem's directions), 1 = more bounds than the instance holds, 3 (after step 4) = a non-positive
//      pivot.  A flagged problem writes its flag (and NaN first moves) and nothing else;
//   3. the lower triangle of S = H64[A, A], packed by rows (row i at i (i + 1) / 2), one wave per row, lanes along the row;
//   4. a right-looking Cholesky S = L L' in place: per column one scaled column (kept in a vector beside the factor) and the rank-1
//      update of the trailing triangle, one wave per row, lanes along the row -- every access to the factor is to a contiguous piece
//      of a packed row;
//   5. in chunks of at most SENS_CHUNK directions: t_A = Kunc64[A, :] dx0, one wave per gathered row, one accumulator per direction,
//      a butterfly over the wave;
//   6. the right-hand sides t_A - du_A;
//   7. L y = r as dot products along the packed rows, L' x = y as updates along them (so the backward pass reads rows too), one wave
//      per pair of right-hand sides (c, c + 4) and no workgroup barrier inside either pass: a wave's LDS operations complete in order;
//   8. lam into the window rows of the caller's LAM (sequence output: du = T - LAM Hinv' follows as two GEMMs and an epilogue), or
//   9. the first moves du_0 = Kunc64[0:nu, :] dx0 - H64[A, 0:nu]' lam, first-stage active entries replaced by the copied perturbation.
// Two instances of the one template: the factor in dynamic LDS for m <= SENS_M_LDS = 160 (12 880 doubles = 103 KB, with the vectors
// 113 KB: one workgroup per CU), and in a slab of global memory per workgroup for 160 < m <= SENS_M_MAX = 768 (the ceiling of
// asm_max_active), where a workgroup walks its share of the launch's list.  Integer data whose partial sums stay below 2^53 and whose
// pivots are even powers of two come out exact: nothing here depends on the order of a sum for such data.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "qp_mult.h"

namespace nnmpc {

constexpr int SENS_THREADS = 256;
constexpr int SENS_CHUNK = 8;        // directions solved together
constexpr int SENS_M_LDS = 160;      // largest set of the LDS instance
constexpr int SENS_M_MAX = 768;      // largest set at all
constexpr size_t SENS_SLAB = (size_t)SENS_M_MAX * (SENS_M_MAX + 1) / 2;   // doubles of a workgroup's slab

template <bool SLAB> constexpr int sens_maxm() { return SLAB ? SENS_M_MAX : SENS_M_LDS; }
template <bool SLAB> constexpr size_t sens_lds_bytes() {
  return ((SLAB ? 0 : (size_t)SENS_M_LDS * (SENS_M_LDS + 1) / 2) + (size_t)(SENS_CHUNK + 1) * sens_maxm<SLAB>()) * 8 + (size_t)sens_maxm<SLAB>() * 4;
}

struct SensArgs {
  const double* H64; const double* Kunc64;   // np x np (symmetric), np x ka
  const uint32_t* active;                    // nprob x words
  const int32_t* status;                     // nprob or nullptr
  const double* dx0;                         // nprob x D x n_aug
  const double* dlb; const double* dub;      // nprob x D x nu each, or nullptr (zeros)
  const int* list; int count;                // the problems of this launch
  double* slab;                              // SLAB instance: SENS_SLAB doubles per workgroup
  double* lam; size_t ldl;                   // sequence output: (nprob D) x ldl, zero on entry; else nullptr
  double* du0;                               // first-move output: (nprob D) x nu; else nullptr
  int32_t* flag;                             // nprob
  int n, np, nu, n_aug, ka, words, D;
};

__device__ __forceinline__ bool sens_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }
__device__ __forceinline__ int sens_tri(int i) { return i * (i + 1) / 2; }

// Both passes of one wave's right-hand sides y1 (and y2), in place.  L: the packed factor, m rows.
template <bool TWO>
__device__ __forceinline__ void sens_subst(const double* L, double* y1, double* y2, int m, int lane) {
  for (int i = 0; i < m; ++i) {
    const double* Li = L + sens_tri(i);
    double s1 = 0.0, s2 = 0.0;
    for (int j = lane; j < i; j += 64) {
      const double l = Li[j];
      s1 = fma(l, y1[j], s1);
      if (TWO) s2 = fma(l, y2[j], s2);
    }
    s1 = mult_wave_sum(s1);
    if (TWO) s2 = mult_wave_sum(s2);
    const double d = Li[i];
    if (lane == 0) {
      y1[i] = (y1[i] - s1) / d;
      if (TWO) y2[i] = (y2[i] - s2) / d;
    }
  }
  for (int i = m - 1; i >= 0; --i) {
    const double* Li = L + sens_tri(i);
    const double d = Li[i];
    const double x1 = y1[i] / d, x2 = TWO ? y2[i] / d : 0.0;
    for (int j = lane; j < i; j += 64) {
      const double l = Li[j];
      y1[j] = fma(-l, x1, y1[j]);
      if (TWO) y2[j] = fma(-l, x2, y2[j]);
    }
    if (lane == 0) {
      y1[i] = x1;
      if (TWO) y2[i] = x2;
    }
  }
}

// Steps 1 to 4, shared with adj_k (qp_adj.h).
// 1. The list of problem b's active variables from its words aw: entry = 2 i + (lower ? 1 : 0), the first sens_maxm<SLAB>() of them in
//    idx.  Returns m, counted beyond what the list holds; `bad` gains "both bits of one variable".  All threads of the workgroup.
template <bool SLAB>
__device__ int sens_list(const uint32_t* aw, int n, int nu, int* idx, int& bad) {
  constexpr int MAXM = sens_maxm<SLAB>();
  __shared__ int scnt[SENS_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int m = 0;
  for (int i0 = 0; i0 < n; i0 += SENS_THREADS) {
    const int i = i0 + tid;
    const int side = i < n ? mult_side(aw, i, nu) : 0;
    bad |= side == 3;
    const unsigned long long bal = __ballot(side != 0);
    if (lane == 0) scnt[wave] = __popcll(bal);
    __syncthreads();
    int base = m, total = 0;
#pragma unroll
    for (int w = 0; w < SENS_THREADS / 64; ++w) { const int c = scnt[w]; base += w < wave ? c : 0; total += c; }
    const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
    if (side != 0 && pos < MAXM) idx[pos] = 2 * i + (side == 2 ? 1 : 0);
    m += total;
    __syncthreads();
  }
  return m;
}
// 2. to 4. The flag from the threads' `bad` and m, then S = H64[A, A] and its factor in L.  Returns the flag, the same in every thread.
template <bool SLAB>
__device__ int sens_factor(const double* H64, int np, int m, int bad, double* L, double* col, const int* idx) {
  constexpr int MAXM = sens_maxm<SLAB>();
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int fl = __syncthreads_or(bad) ? 2 : (m > MAXM ? 1 : 0);
  if (fl == 0) {
    // 3. S = H64[A, A], lower triangle
    for (int i = wave; i < m; i += SENS_THREADS / 64) {
      const double* hr = H64 + (size_t)(idx[i] >> 1) * np;
      double* Li = L + sens_tri(i);
      for (int j = lane; j <= i; j += 64) Li[j] = hr[idx[j] >> 1];
    }
    // 4. Cholesky
    for (int k = 0; k < m; ++k) {
      __syncthreads();                                       // the update of column k - 1 (the gather) is complete
      const double d = L[sens_tri(k) + k];                   // (every thread reads the same value: the exit is uniform)
      if (!(d > 0.0) || !sens_finite(d)) { fl = 3; break; }
      const double s = sqrt(d);
      for (int i = k + 1 + tid; i < m; i += SENS_THREADS) {
        const double c = L[sens_tri(i) + k] / s;
        L[sens_tri(i) + k] = c;
        col[i] = c;
      }
      __syncthreads();
      if (tid == 0) L[sens_tri(k) + k] = s;
      for (int i = k + 1 + wave; i < m; i += SENS_THREADS / 64) {
        const double ci = col[i];
        double* Li = L + sens_tri(i);
        for (int j = k + 1 + lane; j <= i; j += 64) Li[j] = fma(-ci, col[j], Li[j]);
      }
    }
    __syncthreads();
  }
  return fl;
}
// Both substitutions of a chunk of nd right-hand sides (the rows of R), between two workgroup barriers: wave w takes (w, w + 4).
template <bool SLAB>
__device__ __forceinline__ void sens_subst_chunk(const double* L, double* R, int m, int nd) {
  constexpr int MAXM = sens_maxm<SLAB>();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (wave < nd) {
    if (wave + 4 < nd) sens_subst<true>(L, R + wave * MAXM, R + (wave + 4) * MAXM, m, lane);
    else sens_subst<false>(L, R + wave * MAXM, nullptr, m, lane);
  }
  __syncthreads();
}

// One problem.  L: room for the packed factor of sens_maxm<SLAB>() rows; R: SENS_CHUNK x MAXM, col: MAXM, idx: MAXM (LDS).
template <bool SLAB>
__device__ void sens_problem(const SensArgs& a, int b, double* L, double* R, double* col, int* idx) {
  constexpr int MAXM = sens_maxm<SLAB>();
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = a.n, np = a.np, nu = a.nu, n_aug = a.n_aug, ka = a.ka, D = a.D;
  const uint32_t* aw = a.active + (size_t)b * a.words;
  const size_t r0 = (size_t)b * D;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);

  int bad = a.status && a.status[b] == NNMPC_ST_NUMERIC;
  const int m = sens_list<SLAB>(aw, n, nu, idx, bad);
  // 2. the flag
  {
    const double* x = a.dx0 + r0 * n_aug;
    for (size_t i = tid; i < (size_t)D * n_aug; i += SENS_THREADS) bad |= !sens_finite(x[i]);
    for (size_t i = tid; i < (size_t)D * nu; i += SENS_THREADS) {
      if (a.dlb) bad |= !sens_finite(a.dlb[r0 * nu + i]);
      if (a.dub) bad |= !sens_finite(a.dub[r0 * nu + i]);
    }
  }
  const int fl = sens_factor<SLAB>(a.H64, np, m, bad, L, col, idx);
  if (tid == 0) a.flag[b] = fl;
  if (fl != 0) {
    if (a.du0)
      for (size_t i = tid; i < (size_t)D * nu; i += SENS_THREADS) a.du0[r0 * nu + i] = qnan;
    return;
  }

  for (int d0 = 0; d0 < D; d0 += SENS_CHUNK) {
    const int nd = D - d0 < SENS_CHUNK ? D - d0 : SENS_CHUNK;
    const double* x = a.dx0 + (r0 + d0) * n_aug;
    const double* plb = a.dlb ? a.dlb + (r0 + d0) * nu : nullptr;
    const double* pub = a.dub ? a.dub + (r0 + d0) * nu : nullptr;
    // 5., 6. r = Kunc64[A, :] dx0 - du_A
    for (int i = wave; i < m; i += SENS_THREADS / 64) {
      const int e = idx[i], row = e >> 1;
      const double* kr = a.Kunc64 + (size_t)row * ka;
      double acc[SENS_CHUNK];
#pragma unroll
      for (int c = 0; c < SENS_CHUNK; ++c) acc[c] = 0.0;
      for (int k = lane; k < n_aug; k += 64) {
        const double kv = kr[k];
#pragma unroll
        for (int c = 0; c < SENS_CHUNK; ++c)
          if (c < nd) acc[c] = fma(kv, x[(size_t)c * n_aug + k], acc[c]);
      }
      const double* pb = (e & 1) ? plb : pub;
      const int cc = row % nu;
#pragma unroll
      for (int c = 0; c < SENS_CHUNK; ++c) {
        if (c >= nd) break;
        const double t = mult_wave_sum(acc[c]);
        if (lane == 0) R[c * MAXM + i] = t - (pb ? pb[(size_t)c * nu + cc] : 0.0);
      }
    }
    // 7. both substitutions, right-hand sides (wave, wave + 4)
    sens_subst_chunk<SLAB>(L, R, m, nd);
    // 8. lam
    if (a.lam)
      for (int t = tid; t < nd * m; t += SENS_THREADS) {
        const int c = t / m, i = t - c * m;
        a.lam[(r0 + d0 + c) * a.ldl + (idx[i] >> 1)] = R[c * MAXM + i];
      }
    // 9. the first moves
    if (a.du0)
      for (int t = tid; t < nd * nu; t += SENS_THREADS) {
        const int c = t / nu, j = t - c * nu;
        const int side = mult_side(aw, j, nu);
        double v;
        if (side == 1) v = pub ? pub[(size_t)c * nu + j] : 0.0;
        else if (side == 2) v = plb ? plb[(size_t)c * nu + j] : 0.0;
        else {
          const double* kr = a.Kunc64 + (size_t)j * ka;
          double t0 = 0.0, h0 = 0.0;
          for (int k = 0; k < n_aug; ++k) t0 = fma(kr[k], x[(size_t)c * n_aug + k], t0);
          for (int i = 0; i < m; ++i) h0 = fma(a.H64[(size_t)(idx[i] >> 1) * np + j], R[c * MAXM + i], h0);
          v = t0 - h0;
        }
        a.du0[(r0 + d0 + c) * nu + j] = v;
      }
    __syncthreads();                                         // (the right-hand sides are rewritten by the next chunk)
  }
}

template <bool SLAB>
__global__ __launch_bounds__(SENS_THREADS) void sens_k(SensArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sens_sm[];
  constexpr int MAXM = sens_maxm<SLAB>();
  double* L = SLAB ? a.slab + (size_t)blockIdx.x * SENS_SLAB : sens_sm;
  double* R = sens_sm + (SLAB ? 0 : SENS_M_LDS * (SENS_M_LDS + 1) / 2);
  double* col = R + SENS_CHUNK * MAXM;
  int* idx = (int*)(col + MAXM);
  for (int li = blockIdx.x; li < a.count; li += gridDim.x) {
    sens_problem<SLAB>(a, a.list[li], L, R, col, idx);
    __syncthreads();
  }
}

// Per problem the number of active variables (both bits count once) and the largest active variable (-1: none): what the host sorts
// a segment into the two instances by.  One wave per problem.
__global__ __launch_bounds__(256) void sens_count_k(const uint32_t* active, int words, int n, int nu, int nprob, int* cnt) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= nprob) return;
  const uint32_t* aw = active + (size_t)b * words;
  int m = 0, hi = -1;
  for (int i = lane; i < n; i += 64)
    if (mult_side(aw, i, nu) != 0) { ++m; hi = i; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { m += __shfl_xor(m, o, 64); hi = max(hi, __shfl_xor(hi, o, 64)); }
  if (lane == 0) { cnt[2 * b] = m; cnt[2 * b + 1] = hi; }
}

// dx0 (rows x n_aug) -> (mpad x ka), zeros in the padding: the A operand of T = dX0 Kunc64'.
__global__ void sens_pad_k(double* dst, const double* src, size_t rows, int n_aug, int ka, size_t mpad) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = mpad * ka, stride = (size_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    const size_t r = i / ka;
    const int k = (int)(i - r * ka);
    dst[i] = (r < rows && k < n_aug) ? src[r * n_aug + k] : 0.0;
  }
}

// du = T - X, the active entries overwritten by the copied perturbations, NaN rows for flagged problems; one workgroup per row
// (problem b = row / D).  X = nullptr: no problem of the segment has an active bound.  arep (nullable): the problem's active words
// once per row, for the multiplier kernel that runs on the rows.
__global__ __launch_bounds__(256) void sens_epilogue_k(double* du, const double* T, const double* X, size_t ld, const uint32_t* active,
                                                       const int32_t* flag, const double* dlb, const double* dub, uint32_t* arep,
                                                       int n, int nu, int words, int D) {
  const size_t row = blockIdx.x;
  const int b = (int)(row / D);
  const uint32_t* aw = active + (size_t)b * words;
  if (arep)
    for (int w = threadIdx.x; w < words; w += 256) arep[row * words + w] = aw[w];
  double* o = du + row * n;
  if (flag[b] != 0) {
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    for (int i = threadIdx.x; i < n; i += 256) o[i] = qnan;
    return;
  }
  for (int i = threadIdx.x; i < n; i += 256) {
    const int side = mult_side(aw, i, nu), c = i % nu;
    double v;
    if (side == 1) v = dub ? dub[row * nu + c] : 0.0;
    else if (side == 2) v = dlb ? dlb[row * nu + c] : 0.0;
    else v = X ? T[row * ld + i] - X[row * ld + i] : T[row * ld + i];
    o[i] = v;
  }
}

}  // namespace nnmpc
