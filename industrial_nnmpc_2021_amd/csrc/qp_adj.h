// The adjoint (vector-Jacobian) product of the box-QP solution restricted to the delivered active set (gfx950), nnmpc_qp_adjoint:
// the transpose of the map nnmpc_qp_sensitivity evaluates (qp_sens.h).
//
// With the active set A (and its sides) fixed and a cotangent v of the sequence (in first-move mode: of the first stage, the rest zero):
//     w = (Hinv_AA)^-1 (Hinv[A, :] v),     z = v - E_A w,     gx0 = Kunc' z,     gbound = w on A, +0.0 elsewhere,
//     gub_c = sum { w_i : upper bit of i set, i mod nu = c },      glb_c = the same over the lower bits,
// so that <v, du> = <gx0, dx0> + <glb, dlb> + <gub, dub> for every direction of the forward map.  This is the arrangement the kernel
// uses (not w = v_A + M^-1 Hinv[A, F] v_F): the right-hand side is a plain product with rows of Hinv, whatever the set.
//
// adj_k: one workgroup of four waves per problem; all D cotangents of the problem share ONE factorisation.  The list, the flag, the
// gather of S = H64[A, A], its Cholesky factor and the substitutions are qp_sens.h's (sens_list, sens_factor, sens_subst_chunk), and so
// are the two instances (the factor in LDS for m <= 160, in a slab per workgroup for 160 < m <= 768) and the flags: 2 = no answer
// (status NNMPC_ST_NUMERIC, both bits of one variable, a non-finite cotangent in any of the problem's D rows), 1 = more bounds than
// the instance holds, 3 = a non-positive pivot.  A flagged problem writes its flag and quiet NaN into every output row it owns here
// (gx0 of the sequence mode is the host path's epilogue's), and nothing else.  After the factorisation, in chunks of SENS_CHUNK cotangents:
//   sequence mode (vp != nullptr): the right-hand sides Y[row, idx[i]] from the product Y = Vp H64[0:W, :]' the host ran before the
//     kernel; both substitutions; z = v - w in place on the active entries of the padded copy Vp of v (gx0 = Z KuncT' follows as a
//     GEMM and an epilogue);
//   first-move mode: the right-hand sides H64[A, 0:nu] v0 by gather, one thread per list entry, the sum over the stage in its order;
//     both substitutions; gx0 = Kunc64[0:nu, :]' v0 - Kunc64[A, :]' w, threads along the n_aug columns (rows of Kunc64 are read
//     contiguously), the first sum over the stage and the second over the list, each in its order;
//   both: gbound (free entries and active entries are disjoint stores), and gub / glb, one thread per (cotangent, input, side), the sum
//     over the list in its order.
// No atomics: every sum has one order that depends on the problem alone.  Integer data whose partial sums stay below 2^53 and whose
// pivots are even powers of two come out exact.
#pragma once
#include "qp_sens.h"

namespace nnmpc {

struct AdjArgs {
  const double* H64; const double* Kunc64;   // np x np (symmetric), np x ka
  const uint32_t* active;                    // nprob x words
  const int32_t* status;                     // nprob or nullptr
  const double* v;                           // nprob x D x ncol as the caller gave it (ncol = n, first-move mode: nu): the finite check
  const int* list; int count;                // the problems of this launch
  double* slab;                              // SLAB instance: SENS_SLAB doubles per workgroup
  double* vp; const double* y; size_t ld;    // sequence mode: Vp (in: v padded, out: z) and Y, (nprob D) x ld each; else nullptr
  double* gx0;                               // first-move mode: (nprob D) x n_aug; else nullptr
  double* glb; double* gub;                  // (nprob D) x nu each, or nullptr
  double* gbound;                            // (nprob D) x n, or nullptr
  int32_t* flag;                             // nprob
  int n, np, nu, n_aug, ka, words, D;
};

template <bool SLAB>
__device__ void adj_problem(const AdjArgs& a, int b, double* L, double* R, double* col, int* idx) {
  constexpr int MAXM = sens_maxm<SLAB>();
  const int tid = threadIdx.x;
  const int n = a.n, np = a.np, nu = a.nu, n_aug = a.n_aug, ka = a.ka, D = a.D;
  const bool seq = a.vp != nullptr;
  const int ncol = seq ? n : nu;
  const uint32_t* aw = a.active + (size_t)b * a.words;
  const size_t r0 = (size_t)b * D;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);

  int bad = a.status && a.status[b] == NNMPC_ST_NUMERIC;
  const int m = sens_list<SLAB>(aw, n, nu, idx, bad);
  {
    const double* x = a.v + r0 * ncol;
    for (size_t i = tid; i < (size_t)D * ncol; i += SENS_THREADS) bad |= !sens_finite(x[i]);
  }
  const int fl = sens_factor<SLAB>(a.H64, np, m, bad, L, col, idx);
  if (tid == 0) a.flag[b] = fl;
  if (fl != 0) {
    if (a.gx0)
      for (size_t i = tid; i < (size_t)D * n_aug; i += SENS_THREADS) a.gx0[r0 * n_aug + i] = qnan;
    for (size_t i = tid; i < (size_t)D * nu; i += SENS_THREADS) {
      if (a.glb) a.glb[r0 * nu + i] = qnan;
      if (a.gub) a.gub[r0 * nu + i] = qnan;
    }
    if (a.gbound)
      for (size_t i = tid; i < (size_t)D * n; i += SENS_THREADS) a.gbound[r0 * n + i] = qnan;
    return;
  }

  for (int d0 = 0; d0 < D; d0 += SENS_CHUNK) {
    const int nd = D - d0 < SENS_CHUNK ? D - d0 : SENS_CHUNK;
    const size_t row0 = r0 + d0;
    // the right-hand sides Hinv[A, :] v
    if (seq) {
      for (int t = tid; t < nd * m; t += SENS_THREADS) {
        const int c = t / m, i = t - c * m;
        R[c * MAXM + i] = a.y[(row0 + c) * a.ld + (idx[i] >> 1)];
      }
    } else {
      const double* v0 = a.v + row0 * nu;
      for (int i = tid; i < m; i += SENS_THREADS) {
        const double* hr = a.H64 + (size_t)(idx[i] >> 1) * np;
        double acc[SENS_CHUNK];
#pragma unroll
        for (int c = 0; c < SENS_CHUNK; ++c) acc[c] = 0.0;
        for (int j = 0; j < nu; ++j) {
          const double hv = hr[j];
#pragma unroll
          for (int c = 0; c < SENS_CHUNK; ++c)
            if (c < nd) acc[c] = fma(hv, v0[(size_t)c * nu + j], acc[c]);
        }
#pragma unroll
        for (int c = 0; c < SENS_CHUNK; ++c)
          if (c < nd) R[c * MAXM + i] = acc[c];
      }
    }
    sens_subst_chunk<SLAB>(L, R, m, nd);                     // w, in place
    if (seq) {
      // z = v - w on the active entries
      for (int t = tid; t < nd * m; t += SENS_THREADS) {
        const int c = t / m, i = t - c * m;
        double* p = a.vp + (row0 + c) * a.ld + (idx[i] >> 1);
        *p = *p - R[c * MAXM + i];
      }
    } else {
      // gx0 = Kunc64[0:nu, :]' v0 - Kunc64[A, :]' w
      const double* v0 = a.v + row0 * nu;
      for (int k = tid; k < n_aug; k += SENS_THREADS) {
        double t0[SENS_CHUNK], h0[SENS_CHUNK];
#pragma unroll
        for (int c = 0; c < SENS_CHUNK; ++c) t0[c] = h0[c] = 0.0;
        for (int j = 0; j < nu; ++j) {
          const double kv = a.Kunc64[(size_t)j * ka + k];
#pragma unroll
          for (int c = 0; c < SENS_CHUNK; ++c)
            if (c < nd) t0[c] = fma(kv, v0[(size_t)c * nu + j], t0[c]);
        }
        for (int i = 0; i < m; ++i) {
          const double kv = a.Kunc64[(size_t)(idx[i] >> 1) * ka + k];
#pragma unroll
          for (int c = 0; c < SENS_CHUNK; ++c)
            if (c < nd) h0[c] = fma(kv, R[c * MAXM + i], h0[c]);
        }
#pragma unroll
        for (int c = 0; c < SENS_CHUNK; ++c)
          if (c < nd) a.gx0[(row0 + c) * n_aug + k] = t0[c] - h0[c];
      }
    }
    if (a.gbound) {
      for (int t = tid; t < nd * n; t += SENS_THREADS) {
        const int c = t / n, i = t - c * n;
        if (mult_side(aw, i, nu) == 0) a.gbound[(row0 + c) * n + i] = 0.0;
      }
      for (int t = tid; t < nd * m; t += SENS_THREADS) {
        const int c = t / m, i = t - c * m;
        a.gbound[(row0 + c) * n + (idx[i] >> 1)] = R[c * MAXM + i];
      }
    }
    if (a.glb || a.gub)
      for (int t = tid; t < 2 * nd * nu; t += SENS_THREADS) {
        const int lower = t / (nd * nu), u = t - lower * (nd * nu), c = u / nu, j = u - c * nu;
        double* out = lower ? a.glb : a.gub;
        if (!out) continue;
        double s = 0.0;
        for (int i = 0; i < m; ++i) {
          const int e = idx[i];
          if ((e & 1) == lower && (e >> 1) % nu == j) s += R[c * MAXM + i];
        }
        out[(row0 + c) * nu + j] = s;
      }
    __syncthreads();                                         // (the right-hand sides are rewritten by the next chunk)
  }
}

template <bool SLAB>
__global__ __launch_bounds__(SENS_THREADS) void adj_k(AdjArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sens_sm[];
  constexpr int MAXM = sens_maxm<SLAB>();
  double* L = SLAB ? a.slab + (size_t)blockIdx.x * SENS_SLAB : sens_sm;
  double* R = sens_sm + (SLAB ? 0 : SENS_M_LDS * (SENS_M_LDS + 1) / 2);
  double* col = R + SENS_CHUNK * MAXM;
  int* idx = (int*)(col + MAXM);
  for (int li = blockIdx.x; li < a.count; li += gridDim.x) {
    adj_problem<SLAB>(a, a.list[li], L, R, col, idx);
    __syncthreads();
  }
}

// KT[j, k] = Kunc64[k, j] for j < n_aug, zero rows up to kap: the B operand of GX = Z KT'.
__global__ void adj_transpose_k(double* kt, const double* kunc, int np, int ka, int n_aug, int kap) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)kap * np, stride = (size_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    const int j = (int)(i / np), k = (int)(i - (size_t)j * np);
    kt[i] = j < n_aug ? kunc[(size_t)k * ka + j] : 0.0;
  }
}

// gx0 = the leading n_aug columns of GX, quiet NaN rows for flagged problems; one workgroup per row (problem b = row / D).
__global__ __launch_bounds__(256) void adj_epilogue_k(double* gx0, const double* GX, size_t ld, const int32_t* flag, int n_aug, int D) {
  const size_t row = blockIdx.x;
  const bool ok = flag[row / D] == 0;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  for (int k = threadIdx.x; k < n_aug; k += 256) gx0[row * n_aug + k] = ok ? GX[row * ld + k] : qnan;
}

}  // namespace nnmpc
