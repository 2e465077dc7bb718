// Bound multipliers of delivered results (gfx950): mult = -/+ (P u + tq x0) on the active bounds, +0.0 on the free variables.
//
// The solver paths keep their multipliers in different places and in different units -- the LAM rows of the lock-step rounds belong
// to Pinv (and certify through the inverse-error bound without ever forming P u), the device tail's live in LDS, the small kernel's in
// registers, the PDIP polish's in its slabs.  What a caller can check is defined by what was delivered and by P itself:
//     g_i = (P u_b)_i + (tq x0_b)_i,     mult[b, i] = -g_i (upper bound of i active) | +g_i (lower bound active) | +0.0 (free)
// so that P u + q + z_up - z_lo = 0 on the active rows and z >= 0 at an optimum.  The side comes from the active bits (row order of
// the reference's G: stage k = i / nu, c = i % nu; bit k 2nu + c upper, bit k 2nu + nu + c lower), never from the sign of the value: a
// weakly active bound may come back as a tiny negative number and stays attributable.
//
// asm_mult_k: one workgroup of four waves per problem.  It stages the problem's u row (zero-padded to the row length of P; the first
// MULT_U_LDS entries in LDS, what lies beyond is read through L2 -- LDS does not limit n) and its x0 row, finds out whether the row is
// an answer at all, then walks the variables in trips of 256: every thread classifies one variable, free ones are written as +0.0 at
// once, the active ones of the trip are compacted into a list in LDS (wave ballots, no atomics) and the waves take them in turn.  A row
// is one fp64 gathered product: 16-byte loads per lane from row i of P64 (leading dimension np, a multiple of 64: every row starts on
// a 16-byte boundary) and of tq (leading dimension ka), four loads in flight per lane, two fp64 accumulators, a butterfly over the
// wave, one store.  Integer data whose partial sums stay below 2^53 come out exact in any order; for real data
//     |mult - exact| <= (n + n_aug + 2) 2^-53 (|P_i| |u| + |tq_i| |x0|)     (dot product of n + n_aug terms, any order).
// Rows that are no answer -- status NNMPC_ST_NUMERIC, a non-finite u, both bits of one variable set -- are quiet NaN throughout.
// This is a latency and L2 kernel (at the CDU size ~114 rows of 36 KB per problem, all among the leading ~640 rows of P: 23 MB that
// stay in the Infinity Cache), not an MFMA one; it runs after the solve and touches none of its kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nnmpc {

constexpr int MULT_THREADS = 256;
constexpr int MULT_U_LDS = 4608;     // doubles of u staged in LDS (36 KB: the CDU size whole, four workgroups per CU)
constexpr int MULT_X_LDS = 256;      // doubles of x0 staged in LDS

struct MultArgs {
  const double* P64; const double* tq64;    // np x np, np x ka (zero padding)
  const double* x0; const double* u;        // B x n_aug, B x n
  const uint32_t* active;                   // B x words
  const int32_t* status;                    // B or nullptr
  double* mult;                             // B x n
  int n, np, nu, n_aug, ka, words;
};

__device__ __forceinline__ double mult_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// 0 free, 1 upper, 2 lower, 3 both bits set
__device__ __forceinline__ int mult_side(const uint32_t* aw, int i, int nu) {
  const int k = i / nu, c = i - k * nu;
  const int bu = k * 2 * nu + c, bl = bu + nu;
  return (int)((aw[bu >> 5] >> (bu & 31)) & 1u) | (int)(((aw[bl >> 5] >> (bl & 31)) & 1u) << 1);
}

__global__ __launch_bounds__(MULT_THREADS) void asm_mult_k(MultArgs a) {
  __shared__ __attribute__((aligned(16))) double su[MULT_U_LDS];
  __shared__ __attribute__((aligned(16))) double sx[MULT_X_LDS];
  __shared__ int slist[MULT_THREADS];
  __shared__ int scnt[MULT_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = a.n, np = a.np, nu = a.nu, n_aug = a.n_aug, ka = a.ka;
  const double* ug = a.u + (size_t)b * n;
  const double* xg = a.x0 + (size_t)b * n_aug;
  const uint32_t* aw = a.active + (size_t)b * a.words;
  double* mg = a.mult + (size_t)b * n;

  // stage u and x0 (zeros in the padding), and decide whether this row is an answer.  Every variable's bits are read here as well
  // as in the trips below, on purpose: a both-bits variable anywhere makes the WHOLE row NaN, so the decision has to stand before the
  // first trip stores anything (the words are a few hundred bytes, and the second read hits L1).
  int bad = a.status && a.status[b] == NNMPC_ST_NUMERIC;
  const int nul = np < MULT_U_LDS ? np : MULT_U_LDS;
  for (int i = tid; i < nul || i < n; i += MULT_THREADS) {
    const double v = i < n ? ug[i] : 0.0;
    if (i < nul) su[i] = v;
    if (i < n) bad |= !(fabs(v) <= 1.79769313486231570815e308) || mult_side(aw, i, nu) == 3;
  }
  const int nxl = ka < MULT_X_LDS ? ka : MULT_X_LDS;
  for (int i = tid; i < nxl; i += MULT_THREADS) sx[i] = i < n_aug ? xg[i] : 0.0;
  if (__syncthreads_or(bad)) {
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    for (int i = tid; i < n; i += MULT_THREADS) mg[i] = qnan;
    return;
  }

  for (int i0 = 0; i0 < n; i0 += MULT_THREADS) {
    // the trip's active variables, in order: entry = 2 i + (lower ? 1 : 0)
    const int i = i0 + tid;
    const int side = i < n ? mult_side(aw, i, nu) : 0;
    if (i < n && side == 0) mg[i] = 0.0;
    const unsigned long long m = __ballot(side != 0);
    if (lane == 0) scnt[wave] = __popcll(m);
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < MULT_THREADS / 64; ++w) { const int c = scnt[w]; base += w < wave ? c : 0; total += c; }
    if (side != 0) slist[base + __popcll(m & ((1ull << lane) - 1ull))] = 2 * i + (side == 2 ? 1 : 0);
    __syncthreads();
    for (int r = wave; r < total; r += MULT_THREADS / 64) {
      const int e = slist[r], row = e >> 1;
      const double* pr = a.P64 + (size_t)row * np;
      double acc0 = 0.0, acc1 = 0.0;
      // columns held in LDS: 16-byte loads, four in flight per lane
      int c = 2 * lane;
      for (; c + 384 < nul; c += 512) {
        const double2 p0 = *(const double2*)(pr + c), p1 = *(const double2*)(pr + c + 128);
        const double2 p2 = *(const double2*)(pr + c + 256), p3 = *(const double2*)(pr + c + 384);
        const double2 u0 = *(const double2*)(su + c), u1 = *(const double2*)(su + c + 128);
        const double2 u2 = *(const double2*)(su + c + 256), u3 = *(const double2*)(su + c + 384);
        acc0 = fma(p0.x, u0.x, acc0); acc1 = fma(p0.y, u0.y, acc1);
        acc0 = fma(p1.x, u1.x, acc0); acc1 = fma(p1.y, u1.y, acc1);
        acc0 = fma(p2.x, u2.x, acc0); acc1 = fma(p2.y, u2.y, acc1);
        acc0 = fma(p3.x, u3.x, acc0); acc1 = fma(p3.y, u3.y, acc1);
      }
      for (; c < nul; c += 128) {
        const double2 p0 = *(const double2*)(pr + c);
        const double2 u0 = *(const double2*)(su + c);
        acc0 = fma(p0.x, u0.x, acc0); acc1 = fma(p0.y, u0.y, acc1);
      }
      // ... and the columns beyond: u through L2 (rows of u are not 16-byte aligned: scalar loads), none past n
      for (c = nul + 2 * lane; c < n; c += 128) {
        const double2 p0 = *(const double2*)(pr + c);
        acc0 = fma(p0.x, ug[c], acc0);
        if (c + 1 < n) acc1 = fma(p0.y, ug[c + 1], acc1);
      }
      // q_i = tq_i x0
      const double* tr = a.tq64 + (size_t)row * ka;
      for (c = 2 * lane; c < nxl; c += 128) {
        const double2 t0 = *(const double2*)(tr + c);
        const double2 x0v = *(const double2*)(sx + c);
        acc0 = fma(t0.x, x0v.x, acc0); acc1 = fma(t0.y, x0v.y, acc1);
      }
      for (c = nxl + 2 * lane; c < n_aug; c += 128) {
        const double2 t0 = *(const double2*)(tr + c);
        acc0 = fma(t0.x, xg[c], acc0);
        if (c + 1 < n_aug) acc1 = fma(t0.y, xg[c + 1], acc1);
      }
      const double g = mult_wave_sum(acc0 + acc1);
      if (lane == 0) mg[row] = (e & 1) ? g : -g;
    }
    __syncthreads();                    // (the list and the counts are rewritten by the next trip)
  }
}

}  // namespace nnmpc
