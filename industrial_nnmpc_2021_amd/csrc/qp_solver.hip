// Batched box-constrained condensed-QP solver for gfx950 (MI355X).
//
//   min 1/2 u'Pu + (tq x0)'u   s.t.  lb <= u_k <= ub  (k = 0..N-1)
//
// replaces DenseQPRegulator.solve -> cvxopt.solvers.qp of the reference
// (lib/linearMPC.py:495-512) for B independent (x0, lb, ub) at once.
//
// Algorithm per problem (all problems of a wave advance in lock-step "rounds",
// a per-problem state machine on the device decides what each round does):
//   PDIP   Mehrotra predictor-corrector on the reduced KKT system
//          (P + diag(z_u/s_u + z_l/s_l)) du = r, f32 Cholesky (MFMA) + 2 solves,
//          warm-started at the clipped unconstrained minimiser, run only until
//          the active set is identifiable (ipm_tol).
//   POLISH active set from z > s; solve the free block exactly: f32 Cholesky of
//          the masked P + iterative refinement with f64 residuals (P, q in f64),
//          then an f64 KKT check; a failed check updates the set (primal-dual
//          active-set step) and repeats.  status OPTIMAL = KKT verified in f64.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include "../../include/nnmpc.h"
#define ASM_WG_TU (-1)              // the workgroup kernels of qp_wg.h are compiled in qp_wg_kernels.hip: declarations only here
#include "chol_kernels.h"
#include "gemm_kernels.h"
#include "qp_asm.h"
#include "qp_wide.h"
#include "qp_small.h"
#include "qp_predict.h"
#include "qp_mult.h"
#include "qp_sens.h"
#include "qp_adj.h"
#include "dev_res.h"
static constexpr int ASM_SMALL9_LDS_MAX = 100 * 1024;   // dynamic LDS the nine-block instance of asm_small_k may ask for (81 KB at n = 1024, nu = 64)

using namespace nnmpc;

namespace {

enum { PH_INIT = 0, PH_IPM = 1, PH_POLISH = 2, PH_DONE = 3 };
enum { PS_START = 0, PS_CG = 1, PS_CHECK = 2 };
enum { CNT_ACTIVE = 0, CNT_FACTOR = 1, CNT_IPM = 2, CNT_POLISH = 3, CNT_SOLVE = 4 };

constexpr int POLISH_GRACE = 10;   // polish rounds without a new minimum of infeasible indices before single exchanges
struct QpDev {
  int n, np, nu, slots;
  int max_ipm, max_polish, max_refine, stale_max_changes, stale_cg_limit;
  float ipm_tol, delta;
  double refine_tol, bound_tol, stat_tol, pscale;
  const float* pdiag;  // [np] diagonal of the normalised P
  // f32 [slots][np]
  float *u, *zu, *zl, *lbv, *ubv, *q, *PU, *rd, *rhs, *sol, *dua, *dvec, *mask, *uunc;
  // f64 [slots][np]
  double *x, *q64, *PX, *r64, *p64, *v64;   // PX = P64 * v64
  unsigned char* st;  // [slots][np]  0 free, 1 at upper, 2 at lower
  double *lb64, *ub64;        // [slots][nu] bounds of the problem resident in the slot
  // segment-level inputs (problem-indexed) the slots are (re)filled from
  const double *q64_all, *lb_all, *ub_all;   // [seg][np], [seg][nu], [seg][nu]
  const float* uunc_all;                      // [seg][np]
  const unsigned char* guess_all;             // [seg][n] active-set guess (0 free/1 upper/2 lower) or NULL
  int *slot_prob, *age, *next_prob;
  int seg_count, max_rounds;
  int *phase, *f_factor, *f_solve, *istep, *ipm_it, *nfac, *prounds, *rcnt, *psub, *fail, *stale;
  int *pninf, *pgrace;   // polish exchange rule: fewest infeasible indices seen, rounds of grace left (see kkt_check)
  int* ptie;             // polish tie round done (see kkt_check): bounds violated by less than bound_tol were made active once
  float *mu, *gap, *smu, *qscale;
  double* rz;
  int* counters;
  double* u_out;       // [problems][ldu]: the first nout entries of every solution
  int ldu, nout;
  uint32_t* act_out;   // [slots][words]
  int* status_out;     // [slots]
  int* iters_out;      // [slots][2]
  int words;
};

__device__ __forceinline__ float wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double wave_maxd(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}
// All 256 threads must call; result broadcast to all.
__device__ float block_max(float v, float* sh) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}
__device__ float block_sum(float v, float* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
__device__ double block_maxd(double v, double* sh) {
  v = wave_maxd(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}
__device__ double block_sumd(double v, double* sh) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
__device__ int block_sum_i(int v, int* sh) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

#define SLACK_MIN 1e-12f

__device__ void write_outputs(const QpDev& d, int p, int status);

// ---------------------------------------------------------------------------
// Continuous batching: every free (DONE) slot grabs the next unsolved problem of
// the segment and is initialised for the PDIP (warm start = clipped u_unc).
__global__ __launch_bounds__(256) void refill_k(QpDev d) {
  __shared__ float shf[4];
  __shared__ int s_idx;
  const int p = blockIdx.x, tid = threadIdx.x;
  const size_t o = (size_t)p * d.np;
  if (d.phase[p] != PH_DONE) return;
  if (tid == 0) s_idx = atomicAdd(d.next_prob, 1);
  __syncthreads();
  const int idx = s_idx;
  if (idx >= d.seg_count) {
    if (tid == 0) d.slot_prob[p] = -1;
    return;
  }
  const size_t oi = (size_t)idx * d.np;
  if (tid < d.nu) {
    d.lb64[(size_t)p * d.nu + tid] = d.lb_all[(size_t)idx * d.nu + tid];
    d.ub64[(size_t)p * d.nu + tid] = d.ub_all[(size_t)idx * d.nu + tid];
  }
  float qm = 0.f;
  int invalid = 0;
  for (int r = tid; r < d.np; r += 256) {
    if (r < d.n) {
      const int c = r % d.nu;
      invalid |= !(fabs(d.q64_all[oi + r]) <= 1.79e308);   // (fmaxf below would drop a NaN)
      const float lb = (float)d.lb_all[(size_t)idx * d.nu + c], ub = (float)d.ub_all[(size_t)idx * d.nu + c];
      const double q64 = d.q64_all[oi + r];
      const float q = (float)(q64 / d.pscale);
      const float w = ub - lb;
      float u0 = d.uunc_all[oi + r];
      u0 = fminf(fmaxf(u0, lb + 0.05f * w), ub - 0.05f * w);
      d.lbv[o + r] = lb; d.ubv[o + r] = ub; d.q[o + r] = q; d.u[o + r] = u0; d.q64[o + r] = q64;
      qm = fmaxf(qm, fabsf(q));
    } else {
      d.lbv[o + r] = -1.f; d.ubv[o + r] = 1.f; d.q[o + r] = 0.f; d.u[o + r] = 0.f; d.q64[o + r] = 0.0;
    }
    d.zu[o + r] = 0.f; d.zl[o + r] = 0.f;
    d.mask[o + r] = 1.f; d.dvec[o + r] = 0.f; d.rhs[o + r] = 0.f; d.sol[o + r] = 0.f;
    d.dua[o + r] = 0.f; d.rd[o + r] = 0.f; d.x[o + r] = 0.0; d.st[o + r] = 0;
    d.r64[o + r] = 0.0; d.p64[o + r] = 0.0; d.v64[o + r] = 0.0;
  }
  qm = block_max(qm, shf);
  {
    // NaN / Inf in q (i.e. in x0) or a bound pair with lb > ub (or a NaN): not solved at all -- status NUMERIC, u = NaN
    invalid |= !(qm <= 3.0e38f);
    if (tid < d.nu) invalid |= !(d.lb_all[(size_t)idx * d.nu + tid] <= d.ub_all[(size_t)idx * d.nu + tid]);
    invalid = __syncthreads_or(invalid);
    if (invalid) {
      const double qnan = __longlong_as_double(0x7ff8000000000000ll);
      for (int r = tid; r < d.np; r += 256) d.x[o + r] = qnan;
      if (tid == 0) { d.slot_prob[p] = idx; d.fail[p] = 1; d.ipm_it[p] = d.nfac[p] = 0; }
      __syncthreads();
      write_outputs(d, p, NNMPC_ST_NUMERIC);       // the slot stays free (PH_DONE) and takes the next problem next round
      return;
    }
  }
  // (a guess row that starts with 255 means: no guess for this problem)
  const bool warm = d.guess_all != nullptr && d.guess_all[(size_t)idx * d.n] != 255;
  if (warm) {
    // caller-supplied active set (e.g. the shifted set of the previous step of a closed-loop
    // chain): skip the PDIP, start the polish on it; the fp64 KKT check still certifies the result
    for (int r = tid; r < d.n; r += 256) {
      const int c = r % d.nu;
      int s = d.guess_all[(size_t)idx * d.n + r];
      if (s > 2) s = 0;
      const double xv = s == 1 ? d.ub_all[(size_t)idx * d.nu + c]
                      : s == 2 ? d.lb_all[(size_t)idx * d.nu + c] : (double)d.u[o + r];
      d.st[o + r] = (unsigned char)s;
      d.x[o + r] = xv;
      d.v64[o + r] = xv;
    }
  }
  if (tid == 0) {
    d.slot_prob[p] = idx;
    d.age[p] = 0;
    d.qscale[p] = fmaxf(1.f, qm);
    d.phase[p] = warm ? PH_POLISH : PH_INIT;
    d.f_factor[p] = d.f_solve[p] = 0;
    d.ipm_it[p] = d.nfac[p] = d.prounds[p] = d.rcnt[p] = d.psub[p] = d.fail[p] = d.stale[p] = 0;
    d.pninf[p] = 0x7fffffff; d.pgrace[p] = POLISH_GRACE; d.ptie[p] = 0;
    d.mu[p] = d.gap[p] = d.smu[p] = 0.f; d.rz[p] = 0.0;
  }
}
// Start of a segment: every slot is free.
__global__ void reset_slots_k(QpDev d) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < d.slots) {
    d.phase[p] = PH_DONE; d.slot_prob[p] = -1; d.age[p] = 0;
    d.f_factor[p] = d.f_solve[p] = 0;
  }
  if (p == 0) *d.next_prob = 0;
}

__device__ void write_outputs(const QpDev& d, int p, int status) {
  const int tid = threadIdx.x;
  const size_t o = (size_t)p * d.np;
  const size_t pi = (size_t)d.slot_prob[p];
  for (int r = tid; r < d.nout; r += 256) d.u_out[pi * d.ldu + r] = d.x[o + r];
  const int m = 2 * d.n;
  for (int w = tid; w < d.words; w += 256) {
    uint32_t bits = 0;
    for (int b = 0; b < 32; ++b) {
      const int idx = 32 * w + b;
      if (idx < m) {
        const int k = idx / (2 * d.nu), c = idx % (2 * d.nu);
        const int hit = (c < d.nu) ? (d.st[o + k * d.nu + c] == 1) : (d.st[o + k * d.nu + c - d.nu] == 2);
        bits |= (uint32_t)hit << b;
      }
    }
    if (d.act_out) d.act_out[pi * d.words + w] = bits;
  }
  if (tid == 0) {
    if (d.status_out) d.status_out[pi] = d.fail[p] ? NNMPC_ST_NUMERIC : status;
    if (d.iters_out) { d.iters_out[2 * pi] = d.ipm_it[p]; d.iters_out[2 * pi + 1] = d.nfac[p]; }
  }
}

// Preconditioned CG on the free block  P_FF x_F = -(q + P_FA x_A)_F  in f64, the
// f32 Cholesky of the masked, regularised P being the preconditioner M.
// cg_alpha: needs PX = P p.   x += a p, r -= a P p;  returns 1 if another
// preconditioner solve is wanted (rhs = r), 0 if converged (psub -> CHECK, v = x).
__device__ int cg_alpha(const QpDev& d, int p, double* shd) {
  const int tid = threadIdx.x;
  const size_t o = (size_t)p * d.np;
  double pap = 0.0;
  for (int r = tid; r < d.n; r += 256)
    if (d.st[o + r] == 0) pap += d.p64[o + r] * d.PX[o + r];
  pap = block_sumd(pap, shd);
  const double rz = d.rz[p];
  const bool ok = (pap > 0.0) && (rz > 0.0);
  const double a = ok ? rz / pap : 0.0;
  double pm = 0.0, xm = 0.0;
  for (int r = tid; r < d.n; r += 256) {
    if (d.st[o + r] == 0) {
      const double pv = d.p64[o + r];
      const double x = d.x[o + r] + a * pv;
      d.x[o + r] = x;
      d.r64[o + r] -= a * d.PX[o + r];
      pm = fmax(pm, fabs(pv));
      xm = fmax(xm, fabs(x));
    } else {
      xm = fmax(xm, fabs(d.x[o + r]));
    }
  }
  pm = block_maxd(pm, shd);
  xm = block_maxd(xm, shd);
  const int rc = d.rcnt[p] + 1;
  const bool nan = !(a == a) || !(xm == xm);
  // (the step cap ends the PCG on a FRESH factor only: on a reused one it asks for the factor of the current set first, like
  // stale_cg_limit -- otherwise max_refine < stale_cg_limit gives up a slot with the right set as MAXITER)
  const bool capped = rc >= d.max_refine;
  const bool conv = !ok || nan || (fabs(a) * pm <= d.refine_tol * fmax(1.0, xm)) || (capped && !d.stale[p]);
  if (conv) {
    for (int r = tid; r < d.n; r += 256) d.v64[o + r] = d.x[o + r];
  } else {
    for (int r = tid; r < d.n; r += 256) d.rhs[o + r] = d.st[o + r] ? 0.f : (float)d.r64[o + r];
  }
  // PCG on a stale preconditioner that does not converge quickly: factor the current set instead
  const bool refac = !conv && d.stale[p] && (capped || rc >= d.stale_cg_limit);
  if (refac) for (int r = tid; r < d.n; r += 256) d.v64[o + r] = d.x[o + r];
  __syncthreads();
  if (tid == 0) {
    d.rcnt[p] = refac ? 0 : rc;
    if (nan) d.fail[p] = 1;
    if (conv) d.psub[p] = PS_CHECK;
    if (refac) { d.psub[p] = PS_START; d.stale[p] = 0; }
  }
  return (conv || refac) ? 0 : 1;
}
// cg_beta: needs sol = M^-1 r.   p = z + (r'z / rz_old) p,  v = p.
__device__ void cg_beta(const QpDev& d, int p, double* shd) {
  const int tid = threadIdx.x;
  const size_t o = (size_t)p * d.np;
  double rzn = 0.0;
  for (int r = tid; r < d.n; r += 256)
    if (d.st[o + r] == 0) rzn += d.r64[o + r] * (double)d.sol[o + r];
  rzn = block_sumd(rzn, shd);
  const bool first = d.psub[p] == PS_START;
  const double rz = d.rz[p];
  const double beta = (first || !(rz > 0.0)) ? 0.0 : rzn / rz;
  for (int r = tid; r < d.n; r += 256) {
    double pv = 0.0;
    if (d.st[o + r] == 0) pv = (double)d.sol[o + r] + beta * d.p64[o + r];
    d.p64[o + r] = pv;
    d.v64[o + r] = pv;
  }
  __syncthreads();
  if (tid == 0) { d.rz[p] = rzn; d.psub[p] = PS_CG; }
}

// fp64 KKT check of the refined point (PX = P x).  Returns 1 when the slot is finished
// (outputs written, phase DONE); otherwise the active set has been updated, x snapped to
// the new bounds, psub = START, v = x.
__device__ int kkt_check(const QpDev& d, int p, int* shi, double* shd) {
  const int tid = threadIdx.x, n = d.n;
  const size_t o = (size_t)p * d.np;
  int bad = 0;
  double gfree = 0.0;
  for (int r = tid; r < n; r += 256) {
    const int c = r % d.nu;
    const double g = d.PX[o + r] + d.q64[o + r], x = d.x[o + r];
    const double lb = d.lb64[(size_t)p * d.nu + c], ub = d.ub64[(size_t)p * d.nu + c];
    const int s = d.st[o + r];
    // (written so that a NaN fails every test)
    if (s == 0) { bad += !(x <= ub + d.bound_tol) || !(x >= lb - d.bound_tol) || !(fabs(g) <= 1.79e308); gfree = fmax(gfree, fabs(g)); }
    else if (s == 1) bad += !(g < 0.0);   // multiplier -g must be > 0
    else bad += !(g > 0.0);               // multiplier  g must be > 0
  }
  bad = block_sum_i(bad, shi);
  gfree = block_maxd(gfree, shd);
  const int pr = d.prounds[p] + 1;
  // Tie rule ("a bound is active iff its multiplier is > 0", as the oracle and the active-set path have it): a free variable that
  // sits beyond its bound by LESS than bound_tol passes the feasibility test above, but at the exact optimum that bound is active
  // with a tiny positive multiplier.  Once per problem, when everything else is settled, such bounds are made active and the set is
  // solved again; a multiplier that then comes out with the wrong sign drops the bound by the ordinary rule, and it is not
  // re-added (ptie): at most one extra polish round, only for problems that have such a tie.
  if (bad == 0 && pr <= d.max_polish && !d.ptie[p]) {
    int ties = 0;
    for (int r = tid; r < n; r += 256) {
      if (d.st[o + r] != 0) continue;
      const int c = r % d.nu;
      const double x = d.x[o + r];
      const double lb = d.lb64[(size_t)p * d.nu + c], ub = d.ub64[(size_t)p * d.nu + c];
      if (x > ub) { d.st[o + r] = 1; d.x[o + r] = ub; ++ties; }
      else if (x < lb) { d.st[o + r] = 2; d.x[o + r] = lb; ++ties; }
    }
    ties = block_sum_i(ties, shi);
    __syncthreads();
    if (tid == 0) d.ptie[p] = 1;
    if (ties > 0) {
      for (int r = tid; r < n; r += 256) d.v64[o + r] = d.x[o + r];
      if (tid == 0) {
        d.stale[p] = ties <= d.stale_max_changes;
        d.prounds[p] = pr; d.psub[p] = PS_START; d.rcnt[p] = 0;
        d.f_factor[p] = d.f_solve[p] = 0;
      }
      return 0;
    }
  }
  if (bad == 0 || pr > d.max_polish) {
    // stationarity of the free block certifies the refinement itself
    const double gs = d.pscale * (double)d.qscale[p];
    const int ok = bad == 0 && gfree <= d.stat_tol * gs;
    write_outputs(d, p, ok ? NNMPC_ST_OPTIMAL : NNMPC_ST_MAXITER);
    if (tid == 0) { d.phase[p] = PH_DONE; d.f_factor[p] = d.f_solve[p] = 0; }
    return 1;
  }
  // Exchange rule (block principal pivoting with single-exchange fallback, as in asm_update_k): every infeasible
  // index changes sides while their number keeps reaching new minima (POLISH_GRACE rounds of grace), after that only
  // the one with the SMALLEST index (Murty's least-index rule; earliest MPC stage first) -- the all-at-once rule can
  // cycle for ever on ill-conditioned Hessians.
  int single = 0, rsel = -1;
  {
    const int best = d.pninf[p], grace = d.pgrace[p];
    __syncthreads();
    if (bad < best) { if (tid == 0) { d.pninf[p] = bad; d.pgrace[p] = POLISH_GRACE; } }
    else if (grace > 0) { if (tid == 0) d.pgrace[p] = grace - 1; }
    else single = 1;
  }
  if (single) {
    double rm = -1e300;                                      // minus the smallest infeasible index
    for (int r = tid; r < n; r += 256) {
      const int c = r % d.nu;
      const double g = d.PX[o + r] + d.q64[o + r], x = d.x[o + r];
      const double lb = d.lb64[(size_t)p * d.nu + c], ub = d.ub64[(size_t)p * d.nu + c];
      const int s = d.st[o + r];
      const bool inf = s == 0 ? ((x > ub + d.bound_tol) || (x < lb - d.bound_tol)) : (s == 1 ? g >= 0.0 : g <= 0.0);
      if (inf && -(double)r > rm) rm = -(double)r;
    }
    rm = block_maxd(rm, shd);
    rsel = rm > -1e299 ? (int)(-rm) : -1;
  }
  for (int r = tid; r < n; r += 256) {
    const int c = r % d.nu;
    const double g = d.PX[o + r] + d.q64[o + r], x = d.x[o + r];
    const double lb = d.lb64[(size_t)p * d.nu + c], ub = d.ub64[(size_t)p * d.nu + c];
    const int s = d.st[o + r];
    double xn = x;
    if (single && r != rsel) { d.v64[o + r] = xn; continue; }
    if (s == 0) {
      if (x > ub + d.bound_tol) { d.st[o + r] = 1; xn = ub; }
      else if (x < lb - d.bound_tol) { d.st[o + r] = 2; xn = lb; }
    } else if ((s == 1 && g >= 0.0) || (s == 2 && g <= 0.0)) {
      d.st[o + r] = 0;
    }
    d.x[o + r] = xn;
    d.v64[o + r] = xn;
  }
  if (tid == 0) {
    // few changes: keep the previous factor as the PCG preconditioner (a stale SPD
    // preconditioner is still valid; ~1 extra CG step per changed bound, each ~20x
    // cheaper than a factorisation); cg_alpha falls back to a fresh factor if CG stalls
    d.stale[p] = bad <= d.stale_max_changes;
    d.prounds[p] = pr; d.psub[p] = PS_START; d.rcnt[p] = 0;
    d.f_factor[p] = d.f_solve[p] = 0;
  }
  return 0;
}

// Round stage 1: needs PU = P u (f32) for INIT/IPM slots, PX = P x (f64) for POLISH slots.
__global__ __launch_bounds__(256) void stage_pre_k(QpDev d) {
  __shared__ float shf[4];
  __shared__ int shi[4];
  __shared__ double shd[4];
  const int p = blockIdx.x, tid = threadIdx.x;
  const size_t o = (size_t)p * d.np;
  int ph = d.phase[p];
  if (ph == PH_DONE) return;
  const int n = d.n;
  {
    const int age = d.age[p] + 1;   // rounds this problem has been resident
    __syncthreads();
    if (tid == 0) d.age[p] = age;
    if (age > d.max_rounds) {       // budget exhausted: emit the current iterate, uncertified
      if (ph != PH_POLISH) {
        for (int r = tid; r < n; r += 256) { d.x[o + r] = (double)d.u[o + r]; d.st[o + r] = 0; }
        __syncthreads();
      }
      write_outputs(d, p, NNMPC_ST_MAXITER);
      if (tid == 0) { d.phase[p] = PH_DONE; d.f_factor[p] = d.f_solve[p] = 0; }
      return;
    }
  }

  if (ph == PH_INIT) {
    float s = 0.f;
    for (int r = tid; r < n; r += 256) s += fabsf(d.PU[o + r] + d.q[o + r]);
    s = block_sum(s, shf);
    const float mu0 = 0.1f * s / n + 1e-3f;
    for (int r = tid; r < n; r += 256) {
      const float g = d.PU[o + r] + d.q[o + r];
      const float u = d.u[o + r];
      const float su = fmaxf(d.ubv[o + r] - u, SLACK_MIN), sl = fmaxf(u - d.lbv[o + r], SLACK_MIN);
      d.zu[o + r] = fmaxf(-g, 0.f) + mu0 / su;
      d.zl[o + r] = fmaxf(g, 0.f) + mu0 / sl;
    }
    ph = PH_IPM;
  }

  if (ph == PH_IPM) {
    float rdm = 0.f, gs = 0.f;
    for (int r = tid; r < n; r += 256) {
      const float g = d.PU[o + r] + d.q[o + r];
      const float u = d.u[o + r], zu = d.zu[o + r], zl = d.zl[o + r];
      const float su = fmaxf(d.ubv[o + r] - u, SLACK_MIN), sl = fmaxf(u - d.lbv[o + r], SLACK_MIN);
      const float rdv = g + zu - zl;
      d.rd[o + r] = rdv;
      rdm = fmaxf(rdm, fabsf(rdv));
      gs += su * zu + sl * zl;
    }
    rdm = block_max(rdm, shf);
    gs = block_sum(gs, shf);
    const float mu = gs / (2.f * n);
    const int it = d.ipm_it[p];
    const bool nan = !(rdm == rdm) || !(gs == gs);
    const bool conv = (rdm <= d.ipm_tol * d.qscale[p] && mu <= d.ipm_tol * d.qscale[p]) || it >= d.max_ipm || nan;
    if (!conv) {
      for (int r = tid; r < n; r += 256) {
        const float u = d.u[o + r], zu = d.zu[o + r], zl = d.zl[o + r];
        const float su = fmaxf(d.ubv[o + r] - u, SLACK_MIN), sl = fmaxf(u - d.lbv[o + r], SLACK_MIN);
        d.dvec[o + r] = zu / su + zl / sl + d.delta;
        d.mask[o + r] = 1.f;
        d.rhs[o + r] = -(d.PU[o + r] + d.q[o + r]);
      }
      if (tid == 0) {
        d.phase[p] = PH_IPM;
        d.gap[p] = gs; d.mu[p] = mu;
        d.ipm_it[p] = it + 1; d.nfac[p] += 1;
        d.f_factor[p] = 1; d.f_solve[p] = 1; d.istep[p] = 0;
        atomicAdd(&d.counters[CNT_ACTIVE], 1); atomicAdd(&d.counters[CNT_FACTOR], 1);
        atomicAdd(&d.counters[CNT_IPM], 1); atomicAdd(&d.counters[CNT_SOLVE], 1);
      }
      return;
    }
    // ---- PDIP done: guess the active set, start the polish next round
    for (int r = tid; r < n; r += 256) {
      const float u = d.u[o + r], zu = d.zu[o + r], zl = d.zl[o + r];
      const float su = fmaxf(d.ubv[o + r] - u, SLACK_MIN), sl = fmaxf(u - d.lbv[o + r], SLACK_MIN);
      const int c = r % d.nu;
      int s = 0;
      if (!nan) {
        const float pd = d.pdiag[r];
        const bool au = zu > pd * su, al = zl > pd * sl;
        if (au && al) s = (zu * sl > zl * su) ? 1 : 2; else if (au) s = 1; else if (al) s = 2;
      }
      d.st[o + r] = (unsigned char)s;
      const double xv = s == 1 ? d.ub64[(size_t)p * d.nu + c]
                      : s == 2 ? d.lb64[(size_t)p * d.nu + c]
                               : (nan ? 0.0 : (double)u);
      d.x[o + r] = xv;
      d.v64[o + r] = xv;
    }
    if (tid == 0) {
      if (nan) d.fail[p] = 1;
      d.phase[p] = PH_POLISH; d.psub[p] = PS_START; d.rcnt[p] = 0; d.prounds[p] = 0;
      d.f_factor[p] = d.f_solve[p] = 0;
      atomicAdd(&d.counters[CNT_ACTIVE], 1); atomicAdd(&d.counters[CNT_POLISH], 1);
    }
    return;
  }

  // ---- PH_POLISH (PX = P64 * v64, v = x in START / CHECK, v = p in CG)
  int sub = d.psub[p];
  if (sub == PS_CHECK) {
    if (kkt_check(d, p, shi, shd)) return;          // DONE (outputs written)
    if (tid == 0) { atomicAdd(&d.counters[CNT_ACTIVE], 1); atomicAdd(&d.counters[CNT_POLISH], 1); }
    return;                                         // new active set: P x is stale, restart next round
  }
  if (sub == PS_START) {
    // new active set: r = -(P x + q)_F, z = M^-1 r with M = f32 Cholesky of the masked
    // (regularised) P -- freshly factored, or the previous one when only few bounds changed
    const int keep = d.stale[p];
    for (int r = tid; r < n; r += 256) {
      const int s = d.st[o + r];
      const double rr = s ? 0.0 : -(d.PX[o + r] + d.q64[o + r]);
      d.r64[o + r] = rr;
      d.rhs[o + r] = (float)rr;
      if (!keep) { d.mask[o + r] = s ? 0.f : 1.f; d.dvec[o + r] = s ? 1.f : d.delta; }
    }
    if (tid == 0) {
      d.f_factor[p] = !keep; d.f_solve[p] = 1;
      if (!keep) { d.nfac[p] += 1; atomicAdd(&d.counters[CNT_FACTOR], 1); }
      atomicAdd(&d.counters[CNT_ACTIVE], 1); atomicAdd(&d.counters[CNT_POLISH], 1);
      atomicAdd(&d.counters[CNT_SOLVE], 1);
    }
    return;
  }
  // PS_CG carried over from the previous round: the sub-step loop always stops after part B,
  // i.e. the slot is waiting for the next preconditioner solve (rhs = r is already in place).
  if (tid == 0) {
    d.f_factor[p] = 0; d.f_solve[p] = 1;
    atomicAdd(&d.counters[CNT_ACTIVE], 1); atomicAdd(&d.counters[CNT_POLISH], 1);
    atomicAdd(&d.counters[CNT_SOLVE], 1);
  }
}

// Solve sub-step, part A (after a triangular solve): sol = K^-1 rhs is available.
//   IPM  step 0: affine direction -> sigma -> corrector rhs (another solve follows)
//        step 1: combined direction -> step length -> new iterate (done for this round)
//   POLISH: z = sol -> new CG direction p, v = p (P p is computed next)
__global__ __launch_bounds__(256) void stage_sub_a_k(QpDev d) {
  __shared__ float shf[4];
  __shared__ double shd[4];
  const int p = blockIdx.x, tid = threadIdx.x;
  const size_t o = (size_t)p * d.np;
  if (!d.f_solve[p]) return;
  const int ph = d.phase[p], n = d.n;
  if (ph == PH_POLISH) { cg_beta(d, p, shd); return; }
  if (ph != PH_IPM) return;
  if (d.istep[p] == 0) {
  // IPM: affine (predictor) direction -> sigma -> corrector right-hand side
  float t = 0.f;
  for (int r = tid; r < n; r += 256) {
    const float du = d.sol[o + r], u = d.u[o + r], zu = d.zu[o + r], zl = d.zl[o + r];
    const float su = fmaxf(d.ubv[o + r] - u, SLACK_MIN), sl = fmaxf(u - d.lbv[o + r], SLACK_MIN);
    const float dzu = -zu + zu * du / su, dzl = -zl - zl * du / sl;
    t = fmaxf(t, fmaxf(fmaxf(du / su, -du / sl), fmaxf(-dzu / zu, -dzl / zl)));
  }
  t = block_max(t, shf);
  const float a = t > 0.f ? fminf(1.f, 1.f / t) : 1.f;
  float ga = 0.f;
  for (int r = tid; r < n; r += 256) {
    const float du = d.sol[o + r], u = d.u[o + r], zu = d.zu[o + r], zl = d.zl[o + r];
    const float su = fmaxf(d.ubv[o + r] - u, SLACK_MIN), sl = fmaxf(u - d.lbv[o + r], SLACK_MIN);
    const float dzu = -zu + zu * du / su, dzl = -zl - zl * du / sl;
    ga += (su - a * du) * (zu + a * dzu) + (sl + a * du) * (zl + a * dzl);
  }
  ga = block_sum(ga, shf);
  float sg = ga / d.gap[p];
  sg = fminf(1.f, fmaxf(0.f, sg));
  const float smu = sg * sg * sg * d.mu[p];
  for (int r = tid; r < n; r += 256) {
    const float du = d.sol[o + r], u = d.u[o + r], zu = d.zu[o + r], zl = d.zl[o + r];
    const float su = fmaxf(d.ubv[o + r] - u, SLACK_MIN), sl = fmaxf(u - d.lbv[o + r], SLACK_MIN);
    const float dzu = -zu + zu * du / su, dzl = -zl - zl * du / sl;
    d.rhs[o + r] = -d.rd[o + r] + zu - smu / su - du * dzu / su - zl + smu / sl - du * dzl / sl;
    d.dua[o + r] = du;
  }
  if (tid == 0) { d.smu[p] = smu; d.istep[p] = 1; }
    return;
  }
  const float smu = d.smu[p];
  float t = 0.f;
  for (int r = tid; r < n; r += 256) {
    const float du = d.sol[o + r], da = d.dua[o + r], u = d.u[o + r], zu = d.zu[o + r], zl = d.zl[o + r];
    const float su = fmaxf(d.ubv[o + r] - u, SLACK_MIN), sl = fmaxf(u - d.lbv[o + r], SLACK_MIN);
    const float dzua = -zu + zu * da / su, dzla = -zl - zl * da / sl;
    const float rcu = -su * zu + smu + da * dzua, rcl = -sl * zl + smu - da * dzla;
    const float dzu = (rcu + zu * du) / su, dzl = (rcl - zl * du) / sl;
    t = fmaxf(t, fmaxf(fmaxf(du / su, -du / sl), fmaxf(-dzu / zu, -dzl / zl)));
  }
  t = block_max(t, shf);
  const float a = t > 0.f ? fminf(1.f, 0.99f / t) : 1.f;
  for (int r = tid; r < n; r += 256) {
    const float du = d.sol[o + r], da = d.dua[o + r], u = d.u[o + r], zu = d.zu[o + r], zl = d.zl[o + r];
    const float su = fmaxf(d.ubv[o + r] - u, SLACK_MIN), sl = fmaxf(u - d.lbv[o + r], SLACK_MIN);
    const float dzua = -zu + zu * da / su, dzla = -zl - zl * da / sl;
    const float rcu = -su * zu + smu + da * dzua, rcl = -sl * zl + smu - da * dzla;
    const float dzu = (rcu + zu * du) / su, dzl = (rcl - zl * du) / sl;
    d.u[o + r] = u + a * du;
    d.zu[o + r] = fmaxf(zu + a * dzu, 1e-30f);
    d.zl[o + r] = fmaxf(zl + a * dzl, 1e-30f);
  }
  if (tid == 0) d.f_solve[p] = 0;
}

// Solve sub-step, part B (after PX = P v):  POLISH slots only.
//   CG    : x += a p, r -= a P p; converged -> psub = CHECK, v = x (P x is computed next)
//   CHECK : (P x fresh) fp64 KKT check -> DONE, or new active set for the next round
__global__ __launch_bounds__(256) void stage_sub_b_k(QpDev d) {
  __shared__ int shi[4];
  __shared__ double shd[4];
  const int p = blockIdx.x, tid = threadIdx.x;
  if (d.phase[p] != PH_POLISH) return;
  const int sub = d.psub[p];
  if (sub == PS_CG && d.f_solve[p]) {
    const int go = cg_alpha(d, p, shd);
    if (tid == 0) d.f_solve[p] = go;
  } else if (sub == PS_CHECK) {
    kkt_check(d, p, shi, shd);
  }
}

__global__ void f64_to_f32_k(float* dst, const double* src, size_t count) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < count; i += stride) dst[i] = (float)src[i];
}
// x0 [nprob][n_aug] f64 -> padded [rows][ka] f64 and f32
__global__ void pad_x0_k(double* d64, float* d32, const double* src, int nprob, int n_aug, int ka,
                         int rows) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)rows * ka;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    const int p = (int)(i / ka), k = (int)(i % ka);
    const double v = (p < nprob && k < n_aug) ? src[(size_t)p * n_aug + k] : 0.0;
    d64[i] = v;
    d32[i] = (float)v;
  }
}

}  // namespace

// ---------------------------------------------------------------------------
struct nnmpc_qp {
  int device;
  int n, np, nu, n_aug, ka, NB, T, tiles, slots, words;
  nnmpc_qp_opts opts;
  bool have_kunc;
  // shared problem data
  float* Pt;      // tile-packed lower, f32
  float* P32;     // full np x np, f32
  double* P64;    // full np x np, f64
  double* tq64;   // np x ka
  float* Kunc32;  // np x ka
  float* pdiag;   // np, diagonal of P / pscale
  double pscale;  // median diag(P): the f32 PDIP works on P / pscale, q / pscale
  // per-slot workspace
  float* L;
  float* Y;
  float* Dacc;
  unsigned long long* trsv_count;
  QpDev d;
  // shared-inverse active-set path (qp_asm.h)
  bool have_inverse;
  double* H64;      // np x np
  double* Kunc64;   // np x ka
  double *asm_xunc, *asm_x, *asm_scratch;
  int* asm_wflag;
  unsigned char* asm_wmark;
  unsigned char* asm_st;
  int *asm_state, *asm_rounds, *asm_biglist, *asm_status, *asm_binlist, *asm_idxg, *asm_mg, *asm_row, *asm_lrank, *asm_ctot;
  unsigned char *asm_prec, *asm_redo, *asm_alpha, *asm_rowk, *asm_cflag;
  int* asm_carrylist;
  float* H32;
  int *asm_ninf, *asm_hi;
  double tqmax;         // max |tq| entry
  int asm_pool;
  double asm_e1max, asm_e2max;
  // far-field factorisations of the full-width pass (nnmpc_qp_set_farfield), one per window
  struct Far { int W, r, rp; double *U, *Vx, *Vl, *cu; int* kt; double ksum; double efar; };   // ksum: sum of kt over the column tiles
  std::vector<Far> far;
  std::vector<int> far_missing;   // windows of full-width passes that ran in the dense form for want of factors (handed out once each)
  double p_inf = 0.0;       // max row sum of |P|
  // Row spaces ("views") of the active-set rounds: the buffers indexed by the ROW a round hands a running problem (and that round's
  // counters and k-ranges) rather than by the problem.  view[0] has seg_max rows; view[1] is a second, small one for the round that
  // runs beside a full-width pass, view[2] a third of the same size for the iteration after that round, beside the same pass
  // (solve_segment_asm).  Everything indexed by problem is shared.  The counters of all views are one array of ASM_NVIEW ASM_NCNT
  // ints at view[0].counters (read_counters).
  enum { ASM_NVIEW = 3 };
  struct AsmView {
    double *lam = nullptr, *xh = nullptr, *xhw = nullptr, *tnorm = nullptr, *tslack = nullptr;
    float *lam32 = nullptr, *xh32 = nullptr;
    int *rowprob = nullptr, *kblk = nullptr, *counters = nullptr;
    int rows = 0;                    // running problems a round in this view can hold (multiple of 128; 0: no such view)
  };
  AsmView view[ASM_NVIEW];
  int nview = 1;                     // views that have rows: 1 .. ASM_NVIEW, the first nview of them
  // first-set predictor (qp_predict.h): bf16 fragments of Pinv[0:512, 0:512], step sizes; set by nnmpc_qp_set_inverse when the problem is large enough
  struct PredWin { pu32x4* Hf = nullptr; double L = 0.0; int W = 0; };   // L = 1.05 lambda_max(D^-1/2 Pinv_WW D^-1/2); 0: window not available
  PredWin pred[2];              // [0]: 512 columns, 64 problems per workgroup; [1]: 1024 columns, 32 per workgroup (sets that reach further)
  int* pred_cnt = nullptr;      // device counters: [0] asm_extent_k, [1] sum of the workgroups' iterations after the first (asm_predict_k)
  double* asm_work;
  int seg_max;          // problems per segment (q / warm start precomputed per segment)
  double* x0_64;        // [seg_max][ka]
  float* x0_32;
  double* q64_all;      // [seg_max][np]
  float* uunc_all;      // [seg_max][np]
  double *lb_d, *ub_d;  // [seg_max][nu] staging for host inputs
  double* in_stage;     // [seg_max][n_aug]
  hipStream_t stream;
  hipStream_t stream2 = nullptr;     // side streams of the active-set rounds (large-set kernels: the families do not wait for each other)
  hipStream_t stream3 = nullptr, stream4 = nullptr;
  int asm_tail_budget = 50000;       // iterations of asm_tail_k per problem (set in nnmpc_qp_create)
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_join3 = nullptr, ev_join4 = nullptr;
  hipEvent_t ev_wfork = nullptr;                      // fork of a full-width pass that runs on stream4 beside a round ...
  hipEvent_t ev_wide[ASM_NVIEW] = {};                 // ... and its join, one per view: two passes can be in flight (solve_segment_asm)
  // pinned host copies of the active-set pass's read-backs (the round counters, the status of a segment): into pageable memory a
  // "hipMemcpyAsync" is staged and waited for inside the runtime (a blocking wait); pinned, the copy is a packet on the stream and
  // stream_sync polls for it.
  int* pin_cnt = nullptr;            // [ASM_NVIEW ASM_NCNT + 4]: the round counters of all views, then the predictor's iteration sum
  int* pin_st = nullptr;             // [seg_max]
  bool profiling;
  bool gemm_error = false;      // a GEMM was asked for in a form no kernel implements (gemm64): the call in progress fails
  size_t ev_used;               // profiling events of res.pool taken by the call in progress
  bool ev_failed = false;       // one of them could not be created: the call in progress fails at its end (CallScope)
  struct EvRec { int kind; hipEvent_t e0, e1; double flops; };
  std::vector<EvRec> ev_recs;
  nnmpc_qp_stats stats;
  // grow-only slots of the owner
  enum { // staging of a call's arguments (Staging), one per role whichever entry point runs: a handle runs one call at a time.
         // u / du, active words, status, iters, guess, mult / dmult, an x0-shaped input (nnmpc_qp_multipliers, dx0), dlb, dub, flag
         SC_U = 0, SC_ACT, SC_ST, SC_IT, SC_GUESS, SC_MULT, SC_X0, SC_LB, SC_UB, SC_FLAG,
         // compacted copies for the PDIP fallback: live inside a solve, beside the caller's staging
         SC_FB_GUESS, SC_FB_LIST, SC_FB_X0, SC_FB_LB, SC_FB_UB, SC_FB_U, SC_FB_ACT, SC_FB_ST, SC_FB_IT,
         // nnmpc_qp_sensitivity's work: the segment's counts and launch list; the padded dX0, T = dX0 Kunc', LAM, X = LAM Hinv',
         // the active words once per row (for asm_mult_k); the slab instance's factors
         SC_S_CNT, SC_S_LIST, SC_S_XP, SC_S_T, SC_S_LAM, SC_S_X, SC_S_AREP, SC_S_SLAB,
         // nnmpc_qp_adjoint works in the same ones (SC_S_T: the padded V, then Z; SC_S_LAM: Y = V Hinv'; SC_S_X: GX = Z KuncT') and
         // keeps the transposed image of Kunc64 in a slot of its own (kunct_ok: it holds the accepted pair's)
         SC_A_KT,
         // the corrected multipliers the f32 screen keeps for the round after it (AsmDev::stash): seg_max x ASM_MLDS doubles, made by
         // the first call that carries
         SC_CARRY,
         SC_COUNT };
  bool kunct_ok = false;
  DevRes res{SC_COUNT};         // owns every buffer, stream and event below and above
  int ldu, nout;        // layout of the caller's u buffer for the call in progress (nnmpc_qp_solve_batch_ex)
};

namespace {

// Every environment switch of the QP path ("Environment switches"): diagnostics and A/B runs, results are the same
// either way.  The table is read once, when the process first uses it; the three functions after it keep the read times tests rely on.
struct AsmSwitches {
  bool no_fused_wide;   // NNMPC_NO_FUSED_WIDE: A/B of the fused epilogue (the full-width check as a separate kernel)
  bool no_lazy_xunc;    // NNMPC_NO_LAZY_XUNC: x_unc for all columns up front (round 2)
  bool no_farfield;     // NNMPC_NO_FARFIELD: dense form of the full-width pass (A/B)
  bool no_small_gemm;   // NNMPC_NO_SMALL_GEMM: A/B of the 64 x 64 kernel for GEMMs of few tiles (gemm64_choice)
  bool trace;           // NNMPC_TRACE_ROUNDS: the populations of every round, iterations and set sizes per problem of the small pass and the tails
  int refine;           // NNMPC_REFINE, 1: A/B against separate f32 and fp64 rounds ...
  double refine_tol;    // NNMPC_REFINE_TOL, ASM_REFINE_TOL: ... and the residual below which a corrected solve counts as an fp64 solve
  int early64;          // NNMPC_EARLY64, 4: A/B of the rule
  int pred_iters;       // NNMPC_PRED_ITERS, -1: A/B; 0 = off, > 0 that many (overrides opts.asm_predict_iters)
  int pred_wide;        // NNMPC_PRED_WIDE, -1: A/B; 0 / 1 forces the choice of the predictor's window
  int pred_factor;      // NNMPC_PRED_FACTOR, 3: tenths of an iteration per bound x_unc violates (adaptive count)
  int small_grace;      // NNMPC_SMALL_GRACE, ASM_SM_GRACE: iterations of grace of asm_small_k before single exchanges (small_pass)
  int tail_max;         // NNMPC_TAIL_MAX, 256: stragglers go to the device tail at this many running problems; > 1024 doubles the slab pool
};
bool env_set(const char* name) { return getenv(name) != nullptr; }
int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
AsmSwitches read_switches() {
  AsmSwitches w;
  w.no_fused_wide = env_set("NNMPC_NO_FUSED_WIDE"); w.no_lazy_xunc = env_set("NNMPC_NO_LAZY_XUNC"); w.no_farfield = env_set("NNMPC_NO_FARFIELD");
  w.no_small_gemm = env_set("NNMPC_NO_SMALL_GEMM"); w.trace = env_set("NNMPC_TRACE_ROUNDS");
  w.refine = env_int("NNMPC_REFINE", 1); w.early64 = env_int("NNMPC_EARLY64", 4);
  { const char* e = getenv("NNMPC_REFINE_TOL"); w.refine_tol = e ? atof(e) : ASM_REFINE_TOL; }
  w.pred_iters = env_int("NNMPC_PRED_ITERS", -1); w.pred_wide = env_int("NNMPC_PRED_WIDE", -1);
  w.pred_factor = env_int("NNMPC_PRED_FACTOR", 3); w.small_grace = env_int("NNMPC_SMALL_GRACE", ASM_SM_GRACE); w.tail_max = env_int("NNMPC_TAIL_MAX", 256);
  return w;
}
const AsmSwitches& asm_switches() {
  static const AsmSwitches w = read_switches();
  return w;
}
// Read at every call: tests toggle them inside one process.
bool env_no_small() { return env_set("NNMPC_NO_SMALL"); }              // A/B, tests of the rounds at small sizes
bool env_overlap_off() { return env_int("NNMPC_OVERLAP", 1) == 0; }   // A/B runs, 0 = off
bool env_carry_off() { return env_int("NNMPC_CARRY", 1) == 0; }       // A/B runs, 0 = off
bool env_two_views() { return env_int("NNMPC_VIEWS", 3) == 2; }      // A/B runs, 2 = no second iteration beside a pass
// Read at create (tests only): rows of the second and the third row space, dflt when unset.
long long env_overlap_rows(long long dflt) { const char* e = getenv("NNMPC_OVERLAP_ROWS"); return e ? std::max(0, atoi(e) / 128 * 128) : dflt; }

// The next profiling event of the call in progress, recorded on st.  nullptr when none could be created: the record that
// holds it is skipped, and the call fails at its end (ev_failed).
hipEvent_t ev_mark(nnmpc_qp* h, hipStream_t st) {
  hipEvent_t e = nullptr;
  if (h->res.pool_event(h->ev_used, &e)) { h->ev_failed = true; return nullptr; }
  ++h->ev_used;
  hipEventRecord(e, st);
  return e;
}
// What a profiling record times (EvRec::kind): where ev_collect adds it up.
enum EvKind { EV_PANEL = 0, EV_DIAG, EV_TRSV, EV_TOTAL, EV_LAMBDA, EV_GEMM, EV_UPDATE, EV_LAMBDA32, EV_LAMBDA64, EV_SIDE, EV_PREDICT, EV_MULT, EV_SENS, EV_SENS_TOTAL, EV_ADJ, EV_ADJ_TOTAL };
struct EvScope {
  nnmpc_qp* h; int kind; double flops; hipEvent_t e0; hipStream_t st;
  EvScope(nnmpc_qp* h_, EvKind kind_, double flops_, hipStream_t st_ = nullptr) : h(h_), kind(kind_), flops(flops_), e0(nullptr), st(st_ ? st_ : h_->stream) {
    if (h->profiling) e0 = ev_mark(h, st);
  }
  ~EvScope() {
    if (h->profiling) h->ev_recs.push_back({kind, e0, ev_mark(h, st), flops});
  }
};
void ev_collect(nnmpc_qp* h) {
  for (auto& r : h->ev_recs) {
    float ms = 0.f;
    if (!r.e0 || !r.e1) continue;
    hipEventElapsedTime(&ms, r.e0, r.e1);
    if (r.kind == EV_PANEL) { h->stats.panel_ms += ms; h->stats.panel_launches += 1; h->stats.panel_flops += r.flops; }
    else if (r.kind == EV_DIAG) h->stats.diag_ms += ms;
    else if (r.kind == EV_TRSV) h->stats.trsv_ms += ms;
    else if (r.kind == EV_TOTAL) h->stats.total_ms += ms;
    else if (r.kind == EV_LAMBDA) h->stats.asm_lambda_ms += ms;
    else if (r.kind == EV_GEMM) { h->stats.asm_gemm_ms += ms; h->stats.asm_gemm_flops += r.flops; h->stats.asm_gemm_launches += 1; }
    else if (r.kind == EV_UPDATE) h->stats.asm_update_ms += ms;
    else if (r.kind == EV_LAMBDA32) { h->stats.asm_lambda32_ms += ms; h->stats.asm_lambda32_launches += 1; }
    else if (r.kind == EV_LAMBDA64) { h->stats.asm_lambda64_ms += ms; h->stats.asm_lambda64_launches += 1; }
    else if (r.kind == EV_SIDE) h->stats.asm_side_ms += ms;
    else if (r.kind == EV_MULT) { h->stats.mult_ms += ms; h->stats.mult_launches += 1; }
    else if (r.kind == EV_SENS) { h->stats.sens_ms += ms; h->stats.sens_launches += 1; }
    else if (r.kind == EV_SENS_TOTAL) h->stats.sens_total_ms += ms;
    else if (r.kind == EV_ADJ) { h->stats.adj_ms += ms; h->stats.adj_launches += 1; }
    else if (r.kind == EV_ADJ_TOTAL) h->stats.adj_total_ms += ms;
    else if (r.kind == EV_PREDICT) { h->stats.asm_predict_ms += ms; h->stats.asm_predict_flops += r.flops; }   // (launches: counted at the launch, profiling or not)
  }
  h->ev_recs.clear();
  h->ev_used = 0;
}
// One call of an entry point that launches on the handle.  When profiling, and with a `total` kind, the whole call is timed
// from here to finish().  finish(rc) is the end of a call that got there: the profiling records are added up once the stream
// has drained, and an event that could not be created fails the call.  Every other way out drops the call's records and
// its pending ev_failed, so that the next call on the handle starts clean.
struct CallScope {
  nnmpc_qp* h; int total; hipEvent_t e0 = nullptr;
  explicit CallScope(nnmpc_qp* h_, int total_ = -1) : h(h_), total(total_) {
    if (h->profiling && total >= 0) e0 = ev_mark(h, h->stream);
  }
  int finish(int rc) {
    if (h->profiling) {
      if (total >= 0) h->ev_recs.push_back({total, e0, ev_mark(h, h->stream), 0.0});
      const hipError_t e = stream_sync(h->stream);
      if (e == hipSuccess) ev_collect(h);
      else if (!rc) { set_error("stream_sync at the end of the call: %s", hipGetErrorString(e)); rc = NNMPC_EHIP; }
    }
    return h->ev_failed && !rc ? NNMPC_EHIP : rc;           // (ev_mark left the error text)
  }
  ~CallScope() {
    h->ev_recs.clear();
    h->ev_used = 0;
    h->ev_failed = false;
  }
};
// The layout of u for a nested solve (pdip_fallback's compacted copies), the caller's again on the way out.
struct LayoutScope {
  nnmpc_qp* h; int ldu, nout;
  LayoutScope(nnmpc_qp* h_, int ldu_, int nout_) : h(h_), ldu(h_->ldu), nout(h_->nout) { h->ldu = ldu_; h->nout = nout_; }
  ~LayoutScope() { h->ldu = ldu; h->nout = nout; }
};

template <int NB>
void launch_gemm32(hipStream_t s, float* C, size_t ldc, const float* A, size_t lda, const float* B,
                   size_t ldb, int M, int N, int K) {
  dim3 grid(N / NB, M / NB);
  hipLaunchKernelGGL((gemm_nt_f32_k<NB, false, false>), grid, dim3(256), TileCfg<NB>::LDS_FLOATS * 4, s,
                     C, ldc, A, lda, B, ldb, K, (const float*)nullptr);
}
void gemm32(nnmpc_qp* h, float* C, size_t ldc, const float* A, size_t lda, const float* B, size_t ldb,
            int M, int N, int K) {
  if (N % 128 == 0 && M % 128 == 0) launch_gemm32<128>(h->stream, C, ldc, A, lda, B, ldb, M, N, K);
  else launch_gemm32<64>(h->stream, C, ldc, A, lda, B, ldb, M, N, K);
}
// The fp64 NT GEMM of the solves in three parts -- the choice of the kernel and one launch function per kernel -- so that the
// kernel-level test hook (nnmpc_qp_debug_gemm) runs the launch lines a solve runs.
// kblocks: kdyn holds one bound per 64 rows of A (else one for the launch); rowmap: gather / scatter of the rows (gemm64.h)
enum { GEMM64_REFUSED = 0, GEMM64_T128 = 1, GEMM64_K64 = 2 };
int gemm64_choice(int M, int N, int K, bool rowmap) {
  // (fewer 128 x 128 tiles than CUs -- the x_unc product of a chain step: 149 rows -- leave most of the chip idle behind a few
  // long K loops: four times as many 64 x 64 tiles finish sooner)
  const bool few = !asm_switches().no_small_gemm && !rowmap && (M / 128) * (N / 128) < 200;
  if (M % 128 == 0 && N % 128 == 0 && K % G64_KC == 0 && !few) return GEMM64_T128;
  // the 64 x 64 kernel has no gather / scatter of the rows: running it would write the rows of C to the wrong problems.  The one
  // caller with a rowmap (the device tail's x_unc rows) only exists on the 128-grid (`lazy`); anything else is a bug (gemm64 says so).
  return rowmap ? GEMM64_REFUSED : GEMM64_K64;
}
int launch_gemm64_t128(hipStream_t s, double* C, size_t ldc, const double* A, size_t lda, const double* B, size_t ldb, int M, int N, int K,
                       const int* rowphase, int want, const int* kdyn, const int* mdyn, bool kblocks, const int* rowmap) {
  const int ntm = M / 128, ntn = N / 128;
  hipLaunchKernelGGL(gemm_nt_f64_t128_k, dim3(g64_grid(ntm, ntn)), dim3(256), G64_LDS, s, C, ldc, A, lda, B, ldb, K, ntm, ntn,
                     rowphase, want, kdyn, kblocks ? 2 : 0, mdyn, rowmap);
  return g64_grid(ntm, ntn);                               // (workgroups: the hook reports them)
}
int launch_gemm64_k64(hipStream_t s, double* C, size_t ldc, const double* A, size_t lda, const double* B, size_t ldb, int M, int N, int K,
                      const int* rowphase, int want, const int* kdyn, const int* mdyn, bool kblocks) {
  dim3 grid(N / 64, M / 64);
  hipLaunchKernelGGL(gemm_nt_f64_k, grid, dim3(256), 0, s, C, ldc, A, lda, B, ldb, K, rowphase, want, kdyn, mdyn, kblocks ? 1 : 0);
  return (N / 64) * (M / 64);
}
// Returns the kernel that was launched (GEMM64_*; the solves do not look at it).  GEMM64_REFUSED: nothing was launched, the last error
// is set and h->gemm_error makes the call in progress fail at its next check.
int gemm64(nnmpc_qp* h, double* C, size_t ldc, const double* A, size_t lda, const double* B,
           size_t ldb, int M, int N, int K, const int* rowphase = nullptr, int want = 0,
           const int* kdyn = nullptr, const int* mdyn = nullptr, bool kblocks = false, const int* rowmap = nullptr, int* nwg = nullptr) {
  const int which = gemm64_choice(M, N, K, rowmap != nullptr);
  int g = 0;
  if (which == GEMM64_T128) g = launch_gemm64_t128(h->stream, C, ldc, A, lda, B, ldb, M, N, K, rowphase, want, kdyn, mdyn, kblocks, rowmap);
  else if (which == GEMM64_K64) g = launch_gemm64_k64(h->stream, C, ldc, A, lda, B, ldb, M, N, K, rowphase, want, kdyn, mdyn, kblocks);
  else {
    set_error("gemm64: rowmap with a shape off the 128 x 128 / K %% 16 grid (M = %d, N = %d, K = %d)", M, N, K);
    h->gemm_error = true;
  }
  if (nwg) *nwg = g;
  return which;
}
// XH32 = LAM32 Pinv32' at the end of a round: `rows` running f32 problems, W window columns, one k-bound per 64 rows (kdyn).
// The grid rounds `rows` up to whole tiles: A, C and kdyn reach that far.
// NB x NB tiles, NB / 64 bounds per row tile.  launch_xh32 picks the tile as the round does; the test hook also forces it.
template <int NB>
void launch_xh32_nb(hipStream_t s, float* C, size_t ldc, const float* A, size_t lda, const float* B, size_t ldb, int rows, int W, int K,
                    const int* kdyn) {
  hipLaunchKernelGGL((gemm_nt_f32_kdyn_k<NB>), dim3(W / NB, (rows + NB - 1) / NB), dim3(256), TileCfg<NB>::LDS_FLOATS * 4, s,
                     C, ldc, A, lda, B, ldb, K, kdyn, NB / 64);
}
void launch_xh32(hipStream_t s, float* C, size_t ldc, const float* A, size_t lda, const float* B, size_t ldb, int rows, int W, int K,
                 const int* kdyn) {
  if (W % 128 == 0) launch_xh32_nb<128>(s, C, ldc, A, lda, B, ldb, rows, W, K, kdyn);
  else launch_xh32_nb<64>(s, C, ldc, A, lda, B, ldb, rows, W, K, kdyn);
}

template <int NB>
int set_lds_attrs() {
  HIPCHK(hipFuncSetAttribute((const void*)chol_diag_k<NB>, hipFuncAttributeMaxDynamicSharedMemorySize, chol_diag_lds_bytes<NB>()));
  HIPCHK(hipFuncSetAttribute((const void*)chol_panel_k<NB>, hipFuncAttributeMaxDynamicSharedMemorySize, chol_panel_lds_bytes<NB>()));
  HIPCHK(hipFuncSetAttribute((const void*)trsv_k<NB>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
  HIPCHK(hipFuncSetAttribute((const void*)gemm_nt_f32_k<NB, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, TileCfg<NB>::LDS_FLOATS * 4));
  return NNMPC_OK;
}

template <int NB>
void factor_all(nnmpc_qp* h, int nslots, int nfactor) {
  CholArgs a;
  a.n = h->n; a.np = h->np; a.T = h->T; a.tiles = h->tiles;
  a.Pt = h->Pt; a.L = h->L; a.Y = h->Y; a.Dacc = h->Dacc; a.dvec = h->d.dvec; a.mask = h->d.mask;
  a.flag = h->d.f_factor; a.fail = h->d.fail;
  const double nb = NB;
  for (int j = 0; j < h->T; ++j) {
    {
      EvScope es(h, EV_DIAG, 0.0);
      hipLaunchKernelGGL((chol_diag_k<NB>), dim3(nslots), dim3(256), chol_diag_lds_bytes<NB>(), h->stream, a, j);
    }
    const int below = h->T - 1 - j;
    if (below > 0) {
      // algorithmic flops of this launch: per tile 2 NB^2 (j NB) update + NB^3 triangular solve
      // + NB^3 symmetric rank-NB update of the diagonal tile
      const double fl = (double)nfactor * below * (2.0 * nb * nb * (j * nb) + nb * nb * nb + nb * nb * nb);
      EvScope es(h, EV_PANEL, fl);
      hipLaunchKernelGGL((chol_panel_k<NB>), dim3(below, nslots), dim3(256), chol_panel_lds_bytes<NB>(), h->stream, a, j);
    }
  }
}
template <int NB>
void solve_all(nnmpc_qp* h, int nslots, const int* flag) {
  TrsvArgs a;
  a.n = h->n; a.np = h->np; a.T = h->T; a.tiles = h->tiles;
  a.L = h->L; a.Y = h->Y; a.rhs = h->d.rhs; a.sol = h->d.sol; a.flag = flag; a.count = h->trsv_count;
  EvScope es(h, EV_TRSV, 0.0);
  hipLaunchKernelGGL((trsv_k<NB>), dim3(nslots), dim3(256), (h->np + 5 * NB) * 4, h->stream, a);
}
void factor_dispatch(nnmpc_qp* h, int nslots, int nfactor) {
  if (h->NB == 128) factor_all<128>(h, nslots, nfactor); else factor_all<64>(h, nslots, nfactor);
}
void solve_dispatch(nnmpc_qp* h, int nslots, const int* flag) {
  if (h->NB == 128) solve_all<128>(h, nslots, flag); else solve_all<64>(h, nslots, flag);
}

// One segment (<= h->seg_max problems): q and the warm start for the whole
// segment by two GEMMs, then lock-step rounds over the resident slots with
// finished slots refilled from the segment until it is exhausted.
int solve_segment(nnmpc_qp* h, int nprob, const double* x0_dev, const double* lb_dev, const double* ub_dev,
                  const unsigned char* guess_dev, double* u_dev, uint32_t* act_dev, int32_t* st_dev, int32_t* it_dev) {
  QpDev& d = h->d;
  hipStream_t s = h->stream;
  const int rows = h->slots;
  const int segp = ((nprob + 127) / 128) * 128;
  hipLaunchKernelGGL(pad_x0_k, dim3(512), dim3(256), 0, s, h->x0_64, h->x0_32, x0_dev, nprob, h->n_aug, h->ka, segp);
  gemm64(h, h->q64_all, h->np, h->x0_64, h->ka, h->tq64, h->ka, segp, h->np, h->ka);
  if (h->have_kunc) gemm32(h, h->uunc_all, h->np, h->x0_32, h->ka, h->Kunc32, h->ka, segp, h->np, h->ka);
  else HIPCHK(hipMemsetAsync(h->uunc_all, 0, (size_t)segp * h->np * sizeof(float), s));
  d.q64_all = h->q64_all; d.uunc_all = h->uunc_all; d.lb_all = lb_dev; d.ub_all = ub_dev;
  d.seg_count = nprob;
  d.guess_all = guess_dev;
  d.u_out = u_dev; d.act_out = act_dev; d.status_out = st_dev; d.iters_out = it_dev;
  d.ldu = h->ldu; d.nout = h->nout;
  hipLaunchKernelGGL(reset_slots_k, dim3((rows + 255) / 256), dim3(256), 0, s, d);

  int cnt[8];
  bool any_ipm = true, any_polish = guess_dev != nullptr;
  int issued = 0;  // problems handed to slots so far (host mirror of *next_prob, upper bound)
  const int hard_cap = 1000000;
  for (int round = 0; round < hard_cap; ++round) {
    HIPCHK(hipMemsetAsync(d.counters, 0, 8 * sizeof(int), s));
    if (issued < nprob) {
      hipLaunchKernelGGL(refill_k, dim3(rows), dim3(256), 0, s, d);
      any_ipm = true;
      if (guess_dev) any_polish = true;
    }
    if (any_ipm) gemm32(h, d.PU, h->np, d.u, h->np, h->P32, h->np, rows, h->np, h->np);
    if (any_polish) gemm64(h, d.PX, h->np, d.v64, h->np, h->P64, h->np, rows, h->np, h->np, d.phase, PH_POLISH);
    hipLaunchKernelGGL(stage_pre_k, dim3(rows), dim3(256), 0, s, d);
    HIPCHK(hipMemcpyAsync(cnt, d.counters, 8 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&issued, d.next_prob, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(stream_sync(s));
    if (cnt[CNT_ACTIVE] == 0 && issued >= nprob) break;
    any_ipm = cnt[CNT_IPM] > 0;
    any_polish = cnt[CNT_POLISH] > 0;
    h->stats.rounds += 1;
    h->stats.factorizations += cnt[CNT_FACTOR];
    h->stats.ipm_iterations += cnt[CNT_IPM];
    if (cnt[CNT_FACTOR] > 0) factor_dispatch(h, rows, cnt[CNT_FACTOR]);
    if (cnt[CNT_SOLVE] > 0) {
      // solve sub-steps: the two PDIP solves, and PCG steps + KKT check of polishing slots, all
      // inside the round of their factorisation (slots not concerned exit at once)
      const int nsub = cnt[CNT_POLISH] > 0 ? h->opts.sub_steps : 2;
      for (int k = 0; k < nsub; ++k) {
        solve_dispatch(h, rows, d.f_solve);
        hipLaunchKernelGGL(stage_sub_a_k, dim3(rows), dim3(256), 0, s, d);
        if (cnt[CNT_POLISH] > 0) {
          gemm64(h, d.PX, h->np, d.v64, h->np, h->P64, h->np, rows, h->np, h->np, d.phase, PH_POLISH);
          hipLaunchKernelGGL(stage_sub_b_k, dim3(rows), dim3(256), 0, s, d);
        }
      }
    }
  }
  HIPCHK(stream_sync(s));
  HIPCHK(hipGetLastError());
  h->stats.problems += nprob;
  return 0;
}


// One window of the first-set predictor (qp_predict.h): bf16 MFMA fragments of H' = Pinv[0:W, 0:W] diag(t), t_k = 1 / (L Pinv_kk),
// L = lambda_max(D^-1/2 Pinv_WW D^-1/2) (power iteration, 5 % margin: a step that is a little short costs nothing but speed).
// hh: the padded inverse (np x np, host).  Leaves pw.L = 0 when the window does not apply.
template <int NT>
int build_predictor(nnmpc_qp* h, const std::vector<double>& hh, int np, nnmpc_qp::PredWin& pw) {
  constexpr int W = PredCfg<NT>::W, KS = PredCfg<NT>::KS;
  pw.L = 0.0; pw.W = W;
  std::vector<double> dg(W);
  for (int j = 0; j < W; ++j) { dg[j] = hh[(size_t)j * np + j]; if (!(dg[j] > 0.0)) return 0; }
  std::vector<double> v(W, 1.0), u(W), isd(W);
  for (int j = 0; j < W; ++j) isd[j] = 1.0 / std::sqrt(dg[j]);
  double lam = 0.0;
  // (the change per step is no error bound: with the two largest eigenvalues a factor r apart the Rayleigh quotient still lacks
  // ~ change r^2 / (1 - r^2).  Stopping at a change of 1e-6 left L short by 2e-5 on the CDU plant and, at the old cap of 200 steps,
  // by 2.3e-3 on a plant with r = 0.9988 -- inside the 5 % margin, but not the lambda_max the step is documented to be)
  for (int itp = 0; itp < 5000; ++itp) {
    double nv = 0.0;
    for (int i = 0; i < W; ++i) nv += v[i] * v[i];
    nv = std::sqrt(nv);
    for (int i = 0; i < W; ++i) v[i] *= isd[i] / nv;
    for (int i = 0; i < W; ++i) {
      double sacc = 0.0;
      const double* hr = &hh[(size_t)i * np];
      for (int j = 0; j < W; ++j) sacc += hr[j] * v[j];
      u[i] = sacc * isd[i];
    }
    double num = 0.0;
    for (int i = 0; i < W; ++i) num += u[i] * v[i] / isd[i];
    const bool conv = std::fabs(num - lam) <= 1e-9 * std::fabs(num);
    lam = num;
    v = u;
    if (conv && itp > 8) break;
  }
  if (!(lam > 0.0)) return 0;
  const double L = 1.05 * lam;
  std::vector<unsigned short> hf((size_t)W * W);
  auto bf = [](double x) { float f = (float)x; unsigned u32; memcpy(&u32, &f, 4); return (unsigned short)((u32 + 0x7fffu + ((u32 >> 16) & 1u)) >> 16); };
  for (int jt = 0; jt < W / 16; ++jt)
    for (int ks = 0; ks < KS; ++ks)
      for (int lane = 0; lane < 64; ++lane) {
        const int li = lane & 15, lq = lane >> 4;
        for (int e = 0; e < 8; ++e) {
          const int k = 32 * ks + 8 * lq + e;
          hf[pred_frag_index<NT>(jt, ks, lane) * 8 + e] = bf(hh[(size_t)(16 * jt + li) * np + k] / (L * dg[k]));   // H' = H diag(t)
        }
      }
  if (!pw.Hf) { int rc = h->res.alloc((unsigned short**)&pw.Hf, hf.size()); if (rc) return rc; }
  HIPCHK(hipMemcpy(pw.Hf, hf.data(), hf.size() * 2, hipMemcpyHostToDevice));
  pw.L = L;
  return 0;
}

// asm_extent_k over the last quarter of the 512-column window: *count = problems with a bound x_unc violates there (one 4-byte read-back).
int predictor_extent(nnmpc_qp* h, const AsmDev& a, int nprob, int* count) {
  hipStream_t s = h->stream;
  HIPCHK(hipMemsetAsync(h->pred_cnt, 0, 4, s));
  hipLaunchKernelGGL(asm_extent_k, dim3((nprob + 63) / 64), dim3(256), 0, s, a, PRED_W - PRED_W / 4, PRED_W, h->pred_cnt);
  HIPCHK(hipMemcpyAsync(h->pin_cnt, h->pred_cnt, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(stream_sync(s));
  *count = h->pin_cnt[0];
  h->pin_cnt[0] = 0;
  return 0;
}

// The one launch of asm_predict_k (first_sets and nnmpc_qp_debug_predict): its arguments -- the beta schedule, the adaptive
// rule -- and the instance and grid that go with the window and nu.  iters_req: 0 adaptive (every workgroup between 8 and PRED_MAXIT),
// 1 .. PRED_MAXIT fixed.  a: n, np, nu, nseg, lb, ub, xunc (the window's columns formed) and st (zeroed) are read.  *W_out, *MR_out:
// the window, the problems per workgroup; *flops_per_it: the dense count of one iteration of one workgroup.
int launch_predictor(nnmpc_qp* h, const AsmDev& a, int nprob, int iters_req, int wide, int* W_out, int* MR_out, double* flops_per_it) {
  hipStream_t s = h->stream;
  const int iters = iters_req == 0 ? (int)PRED_MAXIT : iters_req;
  PredArgs pa;
  pa.fac10 = asm_switches().pred_factor;
  pa.iters = iters; pa.adaptive = iters_req == 0; pa.itsum = h->profiling ? h->pred_cnt + 1 : nullptr;
  if (h->profiling) HIPCHK(hipMemsetAsync(h->pred_cnt + 1, 0, 4, s));
  double t = 1.0;
  for (int k = 0; k < iters; ++k) { const double tn = 0.5 * (1.0 + std::sqrt(1.0 + 4.0 * t * t)); pa.beta[k] = (float)((t - 1.0) / tn); t = tn; }
  for (int k = iters; k < PRED_MAXIT; ++k) pa.beta[k] = 0.f;
  const bool nu4 = h->nu % 4 == 0;
  const int W = wide ? PRED_W2 : PRED_W, MR = (wide || !nu4) ? 32 : 64;
  pa.Hf = h->pred[wide].Hf;
  // (flops: the dense count -- every k-step of every iteration after the first; the iterations are summed on the device)
  *flops_per_it = 2.0 * W * (double)W * MR;
  *W_out = W; *MR_out = MR;
  h->stats.asm_predict_launches += 1;
  EvScope es(h, EV_PREDICT, 0.0);
  if (wide) hipLaunchKernelGGL((asm_predict_k<8, 2>), dim3((nprob + 31) / 32), dim3(64 * PRED_NW), (pred_lds_bytes<8, 2>(h->nu)), s, a, pa);
  else if (nu4) hipLaunchKernelGGL((asm_predict_k<4, 4>), dim3((nprob + 63) / 64), dim3(64 * PRED_NW), (pred_lds_bytes<4, 4>(h->nu)), s, a, pa);
  else hipLaunchKernelGGL((asm_predict_k<4, 2, false>), dim3((nprob + 31) / 32), dim3(64 * PRED_NW), (pred_lds_bytes<4, 2>(h->nu)), s, a, pa);
  return 0;
}

// ---- The shared-inverse active-set pass over one segment (solve_segment_asm, at the end of this part, holds its loop).
// The state of one call: what its phases below share.
constexpr int NVIEW = nnmpc_qp::ASM_NVIEW;
struct WideStat { bool open; int view, far_rp, skip, cols; double far_ksum; };
struct AsmCall {
  nnmpc_qp* h; hipStream_t s; const AsmSwitches* sw;
  int nprob, segp;
  AsmDev a;                     // the rounds' kernel arguments (asm_args; the row-space fields follow the round's view: set_view)
  int Wx, winit;                // columns x_unc is formed for; the window the first sets are drawn from
  bool lazy, small, tail_only;  // which form the call takes (solve_segment_asm)
  bool defer_cnt;               // a tail-only call reads its counters with the status, at the end
  bool overlap_on;              // a far-field pass may run beside a round
  bool carry_on;                // the f32 screen keeps its corrected multipliers for the round after it (AsmDev::carry)
  bool views3;                  // ... and a second iteration beside the same pass, in the third view
  int vW[NVIEW] = {}, vrows[NVIEW] = {};   // per view: window and fp64 rows of the last round that ran in it
  bool tail_ran[NVIEW] = {};
  int pend = -1;                // the view whose settled rows await the full-width pass (-1: none)
  // the pass whose asm_wide_k ran last: its flops are counted from the scans of the next bins (they count what asm_wide_k marked)
  // (PassLaunch::stat: a pass just launched -- beside a round its asm_wide_k comes after the bins that count the pass before it)
  WideStat wst = {false, 0, 0, 0, 0, 0.0};
  int fft_prev[NVIEW] = {};
  double pred_flops_per_it = 0.0;
  int kprev = 0;                // largest active index of the round before (AsmDev::kref)
};
// A full-width pass as launch_pass left it: what finish_passes needs to decide its problems.
struct PassLaunch { AsmDev ap; int fused_c0; bool inflight; int view; WideStat stat; };   // inflight: on stream4, its asm_wide_k still to come
// The passes in flight, in launch order (stream4 serialises them): at most two, the second launched behind the first.
struct PassFifo {
  PassLaunch pl[2];
  int n = 0;
  bool holds(int v) const { for (int i = 0; i < n; ++i) if (pl[i].view == v) return true; return false; }
};

void set_view(const nnmpc_qp* h, AsmDev& d, int v) {
  const nnmpc_qp::AsmView& V = h->view[v];
  d.lam = V.lam; d.xh = V.xh; d.xhw = V.xhw; d.T = V.xhw; d.tnorm = V.tnorm; d.tslack = V.tslack; d.lam32 = V.lam32; d.xh32 = V.xh32;
  d.rowprob = V.rowprob; d.kblk = V.kblk; d.counters = V.counters;
}
// All views' round counters -> h->pin_cnt, waited for.
int read_counters(nnmpc_qp* h) {
  HIPCHK(hipMemcpyAsync(h->pin_cnt, h->view[0].counters, NVIEW * ASM_NCNT * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(stream_sync(h->stream));
  return 0;
}
// x_unc = Kunc x0 for the columns c.Wx .. Wto - 1: of the first `rows` problems, or (gather) of the problems on the tail's list
void extend_xunc(AsmCall& c, int Wto, int rows, bool gather) {
  nnmpc_qp* h = c.h;
  gemm64(h, h->asm_xunc + c.Wx, h->np, h->x0_64, h->ka, h->Kunc64 + (size_t)c.Wx * h->ka, h->ka, rows, Wto - c.Wx, h->ka,
         nullptr, 0, nullptr, gather ? c.a.counters + ASM_CNT_TAIL : nullptr, false, gather ? h->asm_biglist : nullptr);
  c.a.Wx = Wto;
  if (!gather) c.Wx = Wto;      // (gather: x_unc beyond Wx exists for the tail's problems only)
}
int tail_lds_bytes(const nnmpc_qp* h, const AsmDev& a) {
  return (a.max_active + ASM_TS + ASM_TAIL_AREA) * 8 + ((h->n + 15) / 16) * 16 + ASM_TAIL_EXTRA;
}

// The kernel arguments of the call: everything but the row-space fields (set_view) and what the rounds set as they go.
void asm_args(AsmCall& c, const double* lb_dev, const double* ub_dev, const unsigned char* guess_dev, double* u_dev, uint32_t* act_dev,
              int32_t* it_dev) {
  nnmpc_qp* h = c.h;
  AsmDev& a = c.a;
  const int nprob = c.nprob;
  a.Kunc = h->Kunc64; a.Wx = c.Wx; a.winit = c.winit;
  a.ffU = a.ffVx = a.ffVl = a.ffcu = nullptr; a.ffk = nullptr; a.ffr = a.ffW = 0;
  a.ff_skip = 0; a.ff_err = 0.0; a.ff_efar = 0.0;
  set_view(h, a, 0);
  a.n = h->n; a.np = h->np; a.nu = h->nu; a.nseg = nprob;
  a.max_active = h->opts.asm_max_active; a.max_rounds = h->opts.asm_max_rounds;
  a.bound_tol = h->opts.bound_tol; a.stat_tol = 1e-8; a.pscale = h->pscale;
  a.e1max = h->asm_e1max; a.e2max = h->asm_e2max; a.x0 = h->x0_64; a.ka = h->ka;
  a.H = h->H64; a.lb = lb_dev; a.ub = ub_dev; a.xunc = h->asm_xunc; a.q64 = h->q64_all;
  a.x = h->asm_x; a.px = h->view[0].xh;
  a.st = h->asm_st; a.guess = guess_dev; a.state = h->asm_state; a.rounds = h->asm_rounds;
  a.biglist = h->asm_biglist; a.binlist = h->asm_binlist; a.idxg = h->asm_idxg; a.mg = h->asm_mg; a.row = h->asm_row; a.tqmax = h->tqmax; a.lrank = h->asm_lrank; a.ctot = h->asm_ctot; a.prec = h->asm_prec; a.redo = h->asm_redo; a.rowk = h->asm_rowk; a.H32 = h->H32; a.alpha = h->asm_alpha; a.ninf_best = h->asm_ninf; a.hi = h->asm_hi; a.nkblk = 2 * (h->seg_max / 64 + 2); a.kref = 0; a.use_f32 = h->opts.asm_f32_rounds >= 0; a.wrows = 0; a.wmark = h->asm_wmark; a.wflag = h->asm_wflag; a.W = h->np; a.scratch = h->asm_scratch; a.work = h->asm_work;
  a.u_out = u_dev; a.ldu = h->ldu; a.nout = h->nout; a.act_out = act_dev; a.status_out = h->asm_status; a.iters_out = it_dev; a.words = h->words;
  a.refine = 0; a.refine_later = c.sw->refine && a.use_f32; a.refine_tol = c.sw->refine_tol;
  a.early64 = c.sw->early64;
  a.carry = 0; a.stash = nullptr; a.cflag = h->asm_cflag; a.carrylist = h->asm_carrylist;
  a.pred_w = 0;
}

// First sets: named by the dual projected-gradient predictor inside its window (qp_predict.h), by the bounds x_unc violates beyond
// it (and everywhere when the predictor is off, the problem small, or the caller brought a guess)
int first_sets(AsmCall& c) {
  nnmpc_qp* h = c.h;
  AsmDev& a = c.a;
  const int nprob = c.nprob;
  {
    const int env_it = c.sw->pred_iters;
    // (opts.asm_predict_iters: 0 adaptive, > 0 that many, < 0 off; the variable: 0 off, > 0 that many)
    const int iters_req = env_it >= 0 ? (env_it == 0 ? -1 : std::min(env_it, (int)PRED_MAXIT)) : h->opts.asm_predict_iters;
    const int iters = iters_req == 0 ? (int)PRED_MAXIT : iters_req;
    // (not for the one-wave-per-problem path of small problems: measured on the CSTRs-size batch of 10 000 -- n = 540, nu = 6, cond 4e7 --
    // the prediction takes the mean iteration count from 5.5 to 2, but a launch of asm_small_k lasts as long as its SLOWEST problem, and
    // that one keeps its ~25 iterations: 1.76 ms per step without, 1.94 with the predictor)
    if (iters > 0 && h->pred[0].L > 0.0 && !a.guess && !c.small && !c.tail_only && c.Wx >= PRED_W) {
      // Which window: the optimum's active bounds reach further along the horizon than the bounds x_unc violates.  When more than a
      // quarter of the problems already violate a bound in the last quarter of the 512-column window (CDU plant: 0.05 % at sx = 2,
      // 8 % at sx = 4, 46 % at sx = 6), the 1024-column instance names the sets -- four times the L2 traffic per problem and x_unc
      // for those columns: 100 000 problems at sx = 6 (291 bounds each, the last one at column 757): 461 -> 412 ms per step; at
      // sx = 4 (216 bounds, last column 629) it costs more than it saves (76 -> 88 ms).  (One 4-byte read-back; only handles that
      // have the wide window pay it.)
      int wide = 0;
      if (h->pred[1].L > 0.0 && c.lazy) {
        if (c.sw->pred_wide >= 0) wide = c.sw->pred_wide;
        else {
          int count = 0;
          const int rc = predictor_extent(h, a, nprob, &count);
          if (rc) return rc;
          wide = count * 4 > nprob;
        }
      }
      if (wide && c.Wx < PRED_W2) {
        EvScope es(h, EV_GEMM, 2.0 * (PRED_W2 - c.Wx) * (double)h->ka * nprob);
        extend_xunc(c, PRED_W2, c.segp, false);
      }
      int W = 0, MR = 0;
      const int rc = launch_predictor(h, a, nprob, iters_req, wide, &W, &MR, &c.pred_flops_per_it);
      if (rc) return rc;
      a.pred_w = W;
    }
  }
  hipLaunchKernelGGL(asm_init_k, dim3((c.segp + 3) / 4), dim3(256), 0, c.s, a, c.segp);
  return 0;
}

// ---- NNMPC_TRACE_ROUNDS (diagnostics, AsmSwitches::trace): what the passes print to stderr
std::vector<int> fetch_ints(const int* dev, int n) {
  std::vector<int> v(n);
  hipMemcpy(v.data(), dev, n * sizeof(int), hipMemcpyDeviceToHost);
  return v;
}
std::vector<unsigned char> fetch_bytes(const unsigned char* dev, int n) {
  std::vector<unsigned char> v(n);
  hipMemcpy(v.data(), dev, n, hipMemcpyDeviceToHost);
  return v;
}
// the small pass: iterations and set sizes per problem
int trace_small(AsmCall& c) {
  nnmpc_qp* h = c.h;
  const int nprob = c.nprob;
  HIPCHK(stream_sync(c.s));
  const std::vector<int> rd = fetch_ints(h->asm_rounds, nprob), mg = fetch_ints(h->asm_mg, nprob), stt = fetch_ints(h->asm_state, nprob);
  long sum = 0, sm = 0, big = 0, bigit = 0, left = 0; int mx = 0, mm = 0, mxbig = 0, hist[8] = {0};
  for (int i = 0; i < nprob; ++i) {
    sum += rd[i]; mx = std::max(mx, rd[i]); sm += mg[i]; mm = std::max(mm, mg[i]); left += stt[i] == ASM_RUN;
    if (mg[i] > 32) { ++big; bigit += rd[i]; mxbig = std::max(mxbig, rd[i]); }
    hist[std::min(7, rd[i] / 8)]++;
  }
  fprintf(stderr, "asm small: %d problems, iterations mean %.2f max %d, final sets mean %.1f max %d; sets > 32: %ld (iterations mean %.1f max %d); handed on %ld; iterations/8 histogram",
          nprob, (double)sum / nprob, mx, (double)sm / nprob, mm, big, big ? (double)bigit / big : 0.0, mxbig, left);
  for (int b = 0; b < 8; ++b) fprintf(stderr, " %d", hist[b]);
  fprintf(stderr, "\n");
#ifdef ASM_SM_PROF
  unsigned long long tp[2][8];
  hipMemcpyFromSymbol(tp, HIP_SYMBOL(asm_small_prof), sizeof tp);
  for (int k = 0; k < 2; ++k)
    fprintf(stderr, "  small instance %d clock sums: list %llu, rhs + solve %llu, x window %llu, signs %llu, exchange / loop %llu; iterations %llu\n", k, tp[k][0], tp[k][1], tp[k][2], tp[k][3], tp[k][5], tp[k][6]);
  memset(tp, 0, sizeof tp); hipMemcpyToSymbol(HIP_SYMBOL(asm_small_prof), tp, sizeof tp);
#endif
  return 0;
}
// a tail-only call: iterations per problem
void trace_tail_only(AsmCall& c) {
  const int nprob = c.nprob;
  const std::vector<int> rd = fetch_ints(c.h->asm_rounds, nprob), mg = fetch_ints(c.h->asm_mg, nprob);
  long sum = 0, sm = 0; int mx = 0, mm = 0;
  for (int i = 0; i < nprob; ++i) { sum += rd[i]; mx = std::max(mx, rd[i]); sm += mg[i]; mm = std::max(mm, mg[i]); }
  fprintf(stderr, "asm tail only: %d problems, iterations mean %.2f max %d, active bounds mean %.1f max %d\n", nprob, (double)sum / nprob, mx, (double)sm / nprob, mm);
}
// the populations of a round (cnt: its counters)
void trace_round(int rounds, int beside, const int* cnt) {
  fprintf(stderr, "asm round %d%s: fp64 %d f32 %d last-active %d wide-checked %d big %d big32 %d | fp64 classes", rounds, beside > 1 ? " (beside two passes)" : (beside ? " (beside the pass)" : ""),
          cnt[ASM_CNT_ROWS64], cnt[ASM_CNT_ROWS32], cnt[ASM_CNT_LAST], cnt[ASM_CNT_WIDE + 1], cnt[ASM_CNT_SLAB], cnt[ASM_CNT_BIG32] + cnt[ASM_CNT_BIG32B]);
  for (int b = 0; b < ASM_NBIN; ++b) fprintf(stderr, " %d", cnt[ASM_CNT_F64 + b]);
  fprintf(stderr, " | f32 classes");
  for (int b = 0; b < ASM_NBIN; ++b) fprintf(stderr, " %d", cnt[ASM_CNT_F32 + b]);
  fprintf(stderr, "\n");
}
// the carry: corrected multipliers the f32 screen kept (before its asm_update_k decides which are of use), problems whose round is a copy
int trace_carry(AsmCall& c, int rounds, const int* cnt) {
  HIPCHK(stream_sync(c.s));
  const std::vector<unsigned char> fl = fetch_bytes(c.h->asm_cflag, c.nprob);
  long kept = 0;
  for (int i = 0; i < c.nprob; ++i) kept += fl[i] == 1;
  fprintf(stderr, "asm round %d carry: corrected-and-stashed %ld, carried %d of %d\n", rounds, kept, cnt[ASM_CNT_CARRY], c.nprob);
  return 0;
}
// the tail after a round: iterations of its nrun problems
void trace_tail(AsmCall& c, int rounds, int nrun) {
  const std::vector<int> rd = fetch_ints(c.h->asm_rounds, c.nprob), bl = fetch_ints(c.h->asm_biglist, nrun);
  long sum = 0; int mx = 0;
  for (int i = 0; i < nrun; ++i) { const int r = rd[bl[i]] - rounds; sum += r; mx = std::max(mx, r); }
  fprintf(stderr, "asm tail after round %d: %d problems, iterations mean %.1f max %d\n", rounds, nrun, (double)sum / nrun, mx);
#ifdef ASM_TAIL_PROF
  unsigned long long tp[8];
  hipMemcpyFromSymbol(tp, HIP_SYMBOL(asm_tail_prof), sizeof tp);
  fprintf(stderr, "  tail clock sums (all workgroups): count/factor/solve %llu, substitutions %llu, x loop %llu, tests %llu, exchange %llu; iterations on the dense factor %llu, on a fresh factorisation %llu\n",
          tp[0], tp[1], tp[2], tp[3], tp[4], tp[5], tp[6]);
  memset(tp, 0, sizeof tp); hipMemcpyToSymbol(HIP_SYMBOL(asm_tail_prof), tp, sizeof tp);
#endif
}

// Small problems: the whole iteration in one wave each (qp_small.h), three instances by the size of the set.
int small_pass(AsmCall& c) {
  nnmpc_qp* h = c.h;
  hipStream_t s = c.s;
  const AsmDev& a = c.a;
  const int nprob = c.nprob;
  EvScope es(h, EV_LAMBDA, 0.0);                       // (to the end of the function)
  // iterations of grace before single exchanges (the variable: diagnostics).  24, not the rounds' ASM_GRACE = 10: on the cond-4e7
  // CSTRs-size plant block exchanges that stall for a dozen iterations mostly recover, and a problem sent to single exchanges
  // early pays for it with hundreds of them -- 131 072 problems at sx = 3: 260 ms per step at 10, 78 at 16, 39 at 24, 40 at 40
  // (the ones that truly cycle wait longer for the fallback: 146 ms at 100); the 10 000-problem batch: 47 -> 26 iterations at most
  const int g0 = c.sw->small_grace;
  hipLaunchKernelGGL((asm_small_k<2, 3, 4>), dim3(nprob), dim3(64), asm_small_lds_bytes(2, h->n, h->nu), s, a, a.max_rounds, g0);
  hipLaunchKernelGGL((asm_small_k<7, 1, 8>), dim3(nprob), dim3(64), asm_small_lds_bytes(7, h->n, h->nu), s, a, a.max_rounds, g0);
  // ... and the sets that outgrow its 112 bounds (one problem in two of three 10 000-problem batches of the CSTRs-size plant: handed
  // to the lock-step machinery it cost a round of bookkeeping launches, a read-back and 30 more iterations in the device tail -- 2.7 -
  // 3.1 ms per step against 1.4 without such a problem) carry on in a nine-block instance; a wave whose problem is finished exits at once
  if (asm_small_lds_bytes(9, h->n, h->nu) <= ASM_SMALL9_LDS_MAX)   // (else: handed on as before)
    hipLaunchKernelGGL((asm_small_k<9, 1, 8>), dim3(nprob), dim3(64), asm_small_lds_bytes(9, h->n, h->nu), s, a, a.max_rounds, g0);
  h->stats.asm_rounds += 1;
  h->stats.asm_small_passes += 1;
  return c.sw->trace ? trace_small(c) : 0;
}

// A call of at most 256 problems -- the lock-step chains of a task, a controller's single QP -- is finished on the
// device from the start (asm_tail_k: count -> fp64 solve -> x over all columns -> exchange rule, one workgroup per
// problem): lock-step rounds would be eight launches and a host read-back each for a handful of workgroups.
int tail_only_pass(AsmCall& c) {
  nnmpc_qp* h = c.h;
  hipStream_t s = c.s;
  const AsmDev& a = c.a;
  const int nprob = c.nprob;
  EvScope es(h, EV_LAMBDA, 0.0);                       // (to the end of the function)
  hipLaunchKernelGGL(asm_taillist_k, dim3((nprob + 255) / 256), dim3(256), 0, s, a);
  hipLaunchKernelGGL(asm_tail_k, dim3(nprob), dim3(256), tail_lds_bytes(h, a), s, a, h->asm_tail_budget);
  // (the counters are read together with the status at the end of the segment -- one host round trip per call instead of two:
  // a chain step is such a call, 0.45 ms of which ~0.04 ms was this wait; the check with P is launched unconditionally then)
  if (!c.defer_cnt)
    if (int rc = read_counters(h)) return rc;
  h->stats.asm_rounds += 1;
  if (c.sw->trace) trace_tail_only(c);
  return 0;
}

// Flops of the last full-width pass asm_wide_k has decided (c.wst).  cnt: the counters of the bins pass just read back
void account(AsmCall& c, const int* cnt) {
  nnmpc_qp* h = c.h;
  if (!c.wst.open) return;
  c.wst.open = false;
  if (!h->profiling) return;
  // (the problems asm_wide_k handled, the sum of their last active index + 1)
  const double nw = cnt[ASM_CNT_WIDE + 1], ksum = cnt[ASM_CNT_WKSUM];
  if (c.wst.far_rp) {
    // far-field form: T = z V (k = n_aug + own k-range) and x = T U' (k = the column tile's share of the basis) -- over all
    // columns, or (first-move calls) over the 128 x 128 tiles the certificate did not cover (device count of their k chunks, in
    // the counters of the view the pass ran in)
    const int fft = h->pin_cnt[c.wst.view * ASM_NCNT + ASM_CNT_FFTILES];
    const double chunks = fft - c.fft_prev[c.wst.view];
    c.fft_prev[c.wst.view] = fft;
    h->stats.asm_gemm_flops += 2.0 * c.wst.far_rp * (ksum + nw * h->ka) +
                               (c.wst.skip ? 2.0 * G64_KC * 128.0 * 128.0 * chunks : 2.0 * 128.0 * c.wst.far_ksum * nw);
  } else {
    h->stats.asm_gemm_flops += 2.0 * c.wst.cols * (ksum + (c.lazy ? nw * h->ka : 0.0));   // (lazy: x_unc beyond the window is part of that pass)
  }
}

// The form the pass over view pv takes: its first column c0, fused_c0 (>= 0: the fused kernel's 128-column tiles fit -- the check
// is in the GEMM's epilogue), and the far-field factors of its window if the handle has them (nullptr: a dense form).
const nnmpc_qp::Far* pass_form(const AsmCall& c, int pv, int* c0_out, int* fused_c0_out) {
  const nnmpc_qp* h = c.h;
  const int W = c.vW[pv];   // (that round's window: those columns are in that round's XH rows already)
  const int c0 = (W < h->np && (h->np - W) % 128 == 0) ? W : 0;
  const int fused_c0 = ((h->np - c0) % 128 == 0 && !c.sw->no_fused_wide) ? c0 : -1;
  const nnmpc_qp::Far* ff = nullptr;
  if (c.lazy && fused_c0 > 0 && !c.sw->no_farfield)
    for (const auto& f : h->far) if (f.W == c0) ff = &f;
  *c0_out = c0; *fused_c0_out = fused_c0;
  return ff;
}
// Statistics only: a pass is about to mark its problems while those of the pass before it (c.wst) are still uncounted -- the two may
// be priced differently: count the marks now (scans of the bins in the free view fv; every list and row they write is written again
// by the bins of the next count)
int account_now(AsmCall& c, int fv) {
  nnmpc_qp* h = c.h;
  AsmDev af = c.a;
  set_view(h, af, fv);
  hipLaunchKernelGGL(asm_bins_a_k, dim3((c.nprob + 1023) / 1024), dim3(1024), 0, c.s, af);
  hipLaunchKernelGGL(asm_bins_b_k, dim3((c.nprob + 1023) / 1024), dim3(1024), 0, c.s, af);
  if (int rc = read_counters(h)) return rc;
  account(c, h->pin_cnt + fv * ASM_NCNT);
  return 0;
}
// The full-width pass over the rows of the pending view pv: the problems that settled inside last round's column window get all
// columns of x, once.  On stream4 beside the coming round (pl.inflight: finish_passes decides its problems), else in sequence here.
// behind: a pass is in flight already -- this one queues behind it on stream4 (the loop has made sure it has the far-field form)
int launch_pass(AsmCall& c, int pv, PassLaunch& pl, bool behind) {
  nnmpc_qp* h = c.h;
  hipStream_t s = c.s;
  AsmDev& ap = pl.ap;                                  // the pass's arguments: the pending view, its round's window
  const int prev_rows = c.vrows[pv];
  set_view(h, ap, pv);
  ap.W = c.vW[pv]; ap.wrows = prev_rows;
  pl.view = pv;
  int c0 = 0;
  const nnmpc_qp::Far* ff = pass_form(c, pv, &c0, &pl.fused_c0);
  const int ntm = (prev_rows + 127) / 128, ntn = (h->np - c0) / 128;
  if (c.lazy && pl.fused_c0 > 0 && !c.sw->no_farfield && !ff && h->far_missing.size() < 16 &&
      std::find(h->far_missing.begin(), h->far_missing.end(), c0) == h->far_missing.end())
    h->far_missing.push_back(c0);                  // (the host wrapper may add the factors for this window: nnmpc_qp_farfield_missing)
  const int ov = pv ? 0 : 1;                           // the view a round beside this pass would run in
  const bool ovl = ff && c.overlap_on && h->view[ov].rows > 0;
  if (behind && !ovl) { set_error("launch_pass: a pass behind another one must have the far-field form"); return NNMPC_EINVAL; }
  if (!ovl && c.wst.open && h->profiling && h->view[ov].rows > 0)   // (a pass in sequence after an overlapped one)
    if (int rc = account_now(c, ov)) return rc;
  hipStream_t ps = ovl ? h->stream4 : s;
  if (ovl) {
    HIPCHK(hipEventRecord(h->ev_wfork, s));
    HIPCHK(hipStreamWaitEvent(ps, h->ev_wfork, 0));
  }
  ap.ff_err = 0.0; ap.ff_efar = 0.0; ap.ff_skip = 0;
  int far_rp = 0;
  double far_ksum = 0.0;
  {
    EvScope es(h, EV_GEMM, 0.0, ps);
    if (ff) {
      // far-field form: T = [x0 | lamw] V, x[c0:] = T U'; first-move calls skip the column tiles |U_j| |T_p| certifies
      ap.ffU = ff->U; ap.ffVx = ff->Vx; ap.ffVl = ff->Vl; ap.ffcu = ff->cu; ap.ffk = ff->kt; ap.ffr = ff->rp; ap.ffW = ff->W;
      ap.ff_err = h->p_inf * ff->efar; ap.ff_efar = ff->efar;
      ap.ff_skip = h->nout <= c0 && h->nout < h->n;
      far_rp = ff->rp; far_ksum = ff->ksum;
      h->stats.asm_far_passes += 1;
      hipLaunchKernelGGL(asm_wide_t_k, dim3(g64_grid(ntm, ff->rp / 128)), dim3(256), G64_LDS, ps, ap, ntm, ff->rp / 128);
      if (ap.ff_skip) hipLaunchKernelGGL(asm_wide_tnorm_k, dim3((ntm * 128 + 3) / 4), dim3(256), 0, ps, ap, ntm);
      hipLaunchKernelGGL(asm_wide_gemm_k<WIDE_FAR>, dim3(g64_grid(ntm, ntn)), dim3(256), G64_LDS, ps, ap, c0, ntm, ntn);
    } else if (pl.fused_c0 >= 0 && c.lazy) {              // (lazy: c0 = W >= the first window -- never 0 -- and x_unc exists up to Wx >= W)
      hipLaunchKernelGGL(asm_wide_gemm_k<WIDE_LAZY>, dim3(g64_grid(ntm, ntn)), dim3(256), G64_LDS, s, ap, c0, ntm, ntn);
    } else if (pl.fused_c0 >= 0) {
      hipLaunchKernelGGL(asm_wide_gemm_k<WIDE_XUNC>, dim3(g64_grid(ntm, ntn)), dim3(256), G64_LDS, s, ap, c0, ntm, ntn);
    } else {
      // shapes the fused kernels' tiles do not fit: XHW = LAM Pinv beyond c0 by the plain GEMM, k-range per 64-row block
      gemm64(h, h->view[pv].xhw + c0, h->np, h->view[pv].lam, h->np, h->H64 + (size_t)c0 * h->np, h->np, ((prev_rows + 127) / 128) * 128,
             h->np - c0, h->np, nullptr, 0, h->view[pv].kblk, nullptr, true);
    }
  }
  pl.stat.view = pv; pl.stat.far_rp = far_rp; pl.stat.far_ksum = far_ksum; pl.stat.skip = ap.ff_skip; pl.stat.cols = h->np - c0; pl.stat.open = true;
  if (ovl) {
    HIPCHK(hipEventRecord(h->ev_wide[pv], ps));
    pl.inflight = true;
  } else {
    EvScope es(h, EV_UPDATE, 0.0);
    hipLaunchKernelGGL(asm_wide_k, dim3((prev_rows + 3) / 4), dim3(256), 0, s, ap, pl.fused_c0);
    c.wst = pl.stat;
  }
  c.pend = -1; c.vrows[pv] = 0;
  return 0;
}
// The main stream joins the passes on stream4, in launch order, and decides their problems (rule 1: after everything the iterations
// beside them enqueued)
int finish_passes(AsmCall& c, PassFifo& f) {
  nnmpc_qp* h = c.h;
  for (int i = 0; i < f.n; ++i) {
    PassLaunch& pl = f.pl[i];
    // (statistics only: the first pass's marks are counted before the second one adds its own; its view is free from here on)
    if (i > 0 && c.wst.open && h->profiling)
      if (int rc = account_now(c, f.pl[i - 1].view)) return rc;
    HIPCHK(hipStreamWaitEvent(c.s, h->ev_wide[pl.view], 0));
    EvScope es(h, EV_UPDATE, 0.0);
    hipLaunchKernelGGL(asm_wide_k, dim3((pl.ap.wrows + 3) / 4), dim3(256), 0, c.s, pl.ap, pl.fused_c0);
    c.wst = pl.stat;
    pl.inflight = false;
  }
  f.n = 0;
  return 0;
}

// The round's bookkeeping in view rv: the running problems counted and binned, the counters read back (h->pin_cnt + rv * ASM_NCNT).
// recount: the same problems were counted in the other view already -- the per-problem flop statistics of asm_count_k are not
// added a second time.
int count_round(AsmCall& c, int rv, bool recount) {
  nnmpc_qp* h = c.h;
  hipStream_t s = c.s;
  AsmDev& a = c.a;
  const int nprob = c.nprob;
  set_view(h, a, rv);
  if (recount) a.work = nullptr;
  {
    EvScope es(h, EV_UPDATE, 0.0);                            // set bookkeeping: counted with asm_update_k
    hipLaunchKernelGGL(asm_count_k, dim3((nprob + 3) / 4), dim3(256), 0, s, a);
    hipLaunchKernelGGL(asm_bins_a_k, dim3((nprob + 1023) / 1024), dim3(1024), 0, s, a);
    hipLaunchKernelGGL(asm_bins_b_k, dim3((nprob + 1023) / 1024), dim3(1024), 0, s, a);
  }
  a.work = h->asm_work;
  if (int rc = read_counters(h)) return rc;
  account(c, h->pin_cnt + rv * ASM_NCNT);
  return 0;
}

// The tail: a handful of stragglers (the bulk settles in 5-8 rounds) -- finish them on the device (asm_tail_k)
// instead of paying eight launches and a read-back per round for them.  From round 6 on -- from round 2 when the first sets
// were predicted (qp_predict.h: the bulk then settles in rounds 1-2, and rounds 3-4 were 0.9 ms for 130 problems) -- (12 before: at 100 000
// problems per call the rounds 7..12 were launches for a few dozen problems, 5 % of the step)
int run_tail(AsmCall& c, int rv, int nrun, int rounds, bool inflight) {
  nnmpc_qp* h = c.h;
  hipStream_t s = c.s;
  AsmDev& a = c.a;
  const int nprob = c.nprob;
  {
    EvScope es(h, EV_LAMBDA, 0.0);
    if (c.tail_ran[rv]) HIPCHK(hipMemsetAsync(a.counters + ASM_CNT_TAIL, 0, sizeof(int), s));   // (a second tail of a call, after problems came back from a pass: its own list)
    hipLaunchKernelGGL(asm_taillist_k, dim3((nprob + 255) / 256), dim3(256), 0, s, a);
    // the tail evaluates all columns of its problems straight from Pinv: their x_unc rows beyond Wx, gathered by problem
    if (c.Wx < h->np) extend_xunc(c, h->np, ((nrun + 127) / 128) * 128, true);
    hipLaunchKernelGGL(asm_tail_k, dim3(nrun), dim3(256), tail_lds_bytes(h, a), s, a, h->asm_tail_budget);
    c.tail_ran[rv] = true;
  }
  if (!inflight || c.sw->trace)                          // (beside a pass the next iteration's count reads the counters)
    if (int rc = read_counters(h)) return rc;
  if (c.sw->trace) trace_tail(c, rounds, nrun);
  h->stats.asm_rounds += 1;
  return 0;
}

// The round's multiplier systems, by size class; the large sets on the side streams, joined before the window GEMMs.
// cnt: the round's counters.
int launch_multipliers(AsmCall& c, const int* cnt, bool inflight) {
  nnmpc_qp* h = c.h;
  hipStream_t s = c.s;
  const AsmDev& a = c.a;
  const int lds_big = (a.max_active + ASM_TS) * 8;
  EvScope es(h, EV_LAMBDA, 0.0);
  // one wave per problem, S in registers: size classes 0..5 (<= 144 bounds) in one launch, ASM_REG64_WPB / ASM_REG32_WPB problems
  // per workgroup; classes 6, 7 (<= 176: ASM_REG32B_WPB per workgroup in f32, one workgroup of two waves each in fp64) and the rare larger
  // sets (tiles in an L2 slab, one workgroup each: long latency chains on a handful of CUs) beside it on the side streams.
  const int nwg64s = cnt[ASM_CNT_F64 + 6] + cnt[ASM_CNT_F64 + 7];
  const int nreg32b_wg = asm_reg_wgs<ASM_REG32B_WPB>(cnt[ASM_CNT_F32 + 6]) + asm_reg_wgs<ASM_REG32B_WPB>(cnt[ASM_CNT_F32 + 7]);
  // sets of 177 .. 384 bounds: one workgroup of four or eight waves each (qp_wg.h)
  const int nwg64 = cnt[ASM_CNT_BIG64];
  const int nwg32 = cnt[ASM_CNT_BIG32];
  const int nwg32b = cnt[ASM_CNT_BIG32B];   // f32 rounds of 257 .. 384 bounds: eight waves per problem
  const int nwg64r = cnt[ASM_CNT_BIG64R];   // ... and their fp64 solves: the same factorisation, refined to fp64 residuals
  int nbig = cnt[ASM_CNT_SLAB] + nwg32 + nwg64s + nreg32b_wg + nwg64 + nwg32b + nwg64r, nreg_wg = 0, nreg32_wg = 0;
  for (int b = 0; b < ASM_NREG; ++b) { nreg_wg += asm_reg_wgs<ASM_REG64_WPB>(cnt[ASM_CNT_F64 + b]); nreg32_wg += asm_reg_wgs<ASM_REG32_WPB>(cnt[ASM_CNT_F32 + b]); }
  // three side streams: [slab kernel: few workgroups, long chains -- it starts first and runs beside everything else],
  // [four- and eight-wave kernels of the 12 .. 24-block sets], [kernels of the 10- and 11-block classes]
  // (beside a pass stream4 carries the pass: the slab kernel then goes first on stream2)
  const bool side4 = cnt[ASM_CNT_SLAB] > 0, side2 = nwg64 + nwg32 + nwg32b + nwg64r > 0, side3 = nwg64s + nreg32b_wg > 0;
  hipStream_t st4 = inflight ? h->stream2 : h->stream4;
  if (nbig) {
    HIPCHK(hipEventRecord(h->ev_fork, s));
    if (side4) {
      HIPCHK(hipStreamWaitEvent(st4, h->ev_fork, 0));
      { EvScope e9(h, EV_SIDE, 0.0, st4); hipLaunchKernelGGL((asm_lambda_tile_k<1>), dim3(std::min(cnt[ASM_CNT_SLAB], h->asm_pool)), dim3(256), lds_big, st4, a, 0); }
      HIPCHK(hipEventRecord(h->ev_join4, st4));
    }
    if (side2) {
      HIPCHK(hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
      EvScope e9(h, EV_SIDE, 0.0, h->stream2);
      if (nwg64) hipLaunchKernelGGL(asm_lambda_wg64_k, dim3(nwg64), dim3(256), asm_wg_lds_bytes<double>(), h->stream2, a);
      if (nwg64r) hipLaunchKernelGGL(asm_lambda_wg64r_k, dim3(nwg64r), dim3(512), (asm_wg_lds_bytes_refine<float, ASM_WG_MB8>()), h->stream2, a);
      if (nwg32b) hipLaunchKernelGGL(asm_lambda_wg32b_k, dim3(nwg32b), dim3(512), (asm_wg_lds_bytes<float, ASM_WG_MB8>()), h->stream2, a);
      if (nwg32) hipLaunchKernelGGL(asm_lambda_wg32_k, dim3(nwg32), dim3(256), asm_wg_lds_bytes<float>(), h->stream2, a);
      HIPCHK(hipEventRecord(h->ev_join, h->stream2));
    }
    if (side3) {
      HIPCHK(hipStreamWaitEvent(h->stream3, h->ev_fork, 0));
      EvScope e9(h, EV_SIDE, 0.0, h->stream3);
      // fp64, 145 .. 176 bounds: two waves per problem (7.3 / 5.2 problems per microsecond at 160 / 176 bounds against the 6.0 / 4.5
      // of one wave per problem; in f32 the single-wave kernel wins, 18.1 against 14.3)
      if (nwg64s) hipLaunchKernelGGL(asm_lambda_wg64s_k, dim3(nwg64s), dim3(128), asm_wg_lds_bytes<double>(), h->stream3, a);
      if (nreg32b_wg) hipLaunchKernelGGL(asm_lambda_reg32b_k, dim3(nreg32b_wg), dim3(64 * ASM_REG32B_WPB), ASM_REG32B_LDS, h->stream3, a);
      HIPCHK(hipEventRecord(h->ev_join3, h->stream3));
    }
  }
  // fp64 first (its waves are the long ones), then the f32 rounds of the problems whose set still moves
  if (nreg_wg) { EvScope e8(h, EV_LAMBDA64, 0.0); hipLaunchKernelGGL(asm_lambda_reg_k, dim3(nreg_wg), dim3(64 * ASM_REG64_WPB), ASM_REG_LDS, s, a); }
  // (... and, at the end of that grid, the problems whose solve the round before already did: a copy -- asm_carry_copy)
  nreg32_wg += asm_reg_wgs<ASM_CARRY_GROUP>(cnt[ASM_CNT_CARRY]);
  if (nreg32_wg) { EvScope e7(h, EV_LAMBDA32, 0.0); hipLaunchKernelGGL(asm_lambda_reg32_k, dim3(nreg32_wg), dim3(64 * ASM_REG32_WPB), ASM_REG32_LDS, s, a); }
  if (side2) HIPCHK(hipStreamWaitEvent(s, h->ev_join, 0));
  if (side3) HIPCHK(hipStreamWaitEvent(s, h->ev_join3, 0));
  if (side4) HIPCHK(hipStreamWaitEvent(s, h->ev_join4, 0));
  return 0;
}

// The round's window GEMMs (XH = LAM Pinv' over a.W columns, fp64 and f32 rows) and its set update.  cnt: the round's counters.
int window_gemms_and_update(AsmCall& c, int rv, int n64, int n32, const int* cnt) {
  nnmpc_qp* h = c.h;
  hipStream_t s = c.s;
  const AsmDev& a = c.a;
  const int nprob = c.nprob;
  const nnmpc_qp::AsmView& V = h->view[rv];
  {
    // the running problems sit in rows 0..n64-1 of LAM (fp64 solves) and 0..n32-1 of LAM32 (f32 solves), the rest
    // of the last row block is zero; algorithmic flops of LAM * Pinv: 2 * columns * (k up to the last active bound)
    // per running problem
    // algorithmic flops: 2 * window columns * (own last active bound + 1) per running problem (cnt[ASM_CNT_KSUM] is their sum)
    EvScope es(h, EV_GEMM, 2.0 * a.W * (double)cnt[ASM_CNT_KSUM]);
    if (n64)
      gemm64(h, V.xh, h->np, V.lam, h->np, h->H64, h->np, ((n64 + 127) / 128) * 128, a.W, h->np, nullptr, 0,
             V.kblk, nullptr, true);
    // (rows are ordered by their last active stage: every 64-row block has its own k-range, asm_bins_b_k)
    if (n32)
      launch_xh32(s, V.xh32, (size_t)h->np, V.lam32, (size_t)h->np, h->H32, (size_t)h->np, n32, a.W, h->np, V.kblk + a.nkblk / 2);
  }
  {
    EvScope es(h, EV_UPDATE, 0.0);
    // (rows of LAM whose problem settles inside the window are marked for the full-width pass that opens the next round)
    if (n64) HIPCHK(hipMemsetAsync(V.rowprob, 0xFF, (size_t)((n64 + 127) / 128) * 128 * sizeof(int), s));
    hipLaunchKernelGGL(asm_update_k, dim3((nprob + 3) / 4), dim3(256), 0, s, a);
  }
  return 0;
}

// Problems finished but not certified by the inverse-error bound, counted in the view a problem finished in (h->pin_cnt)
int ndone(const nnmpc_qp* h) {
  int t = 0;
  for (int v = 0; v < NVIEW; ++v) t += h->pin_cnt[v * ASM_NCNT + ASM_CNT_DONE];
  return t;
}
// Certification with P itself (rows the inverse-error bound could not certify): q = tq x0 and px = x P; the status of the segment
// read back (h->pin_st) and handed to the caller.  fb: the problems left for the PDIP path (status 3).
// capped: the loop was left by the round cap -- the last counters are not final.
int certify_and_collect(AsmCall& c, bool capped, int32_t* st_dev, std::vector<int>& fb) {
  nnmpc_qp* h = c.h;
  hipStream_t s = c.s;
  AsmDev& a = c.a;
  const int nprob = c.nprob, segp = c.segp;
  if (capped)
    if (int rc = read_counters(h)) return rc;
  if (h->gemm_error) { h->gemm_error = false; return NNMPC_EINVAL; }
  set_view(h, a, 0);
  if (!c.defer_cnt) h->stats.asm_full_checks += ndone(h);
  if (c.defer_cnt || ndone(h) > 0) {             // (row blocks without an ASM_DONE row leave these GEMMs at once)
    gemm64(h, h->q64_all, h->np, h->x0_64, h->ka, h->tq64, h->ka, segp, h->np, h->ka, h->asm_state, ASM_DONE);
    gemm64(h, h->view[0].xh, h->np, h->asm_x, h->np, h->P64, h->np, segp, h->np, h->np, h->asm_state, ASM_DONE);
  }
  hipLaunchKernelGGL(asm_certify_k, dim3(nprob), dim3(256), 0, s, a, h->pscale);
  int* st = h->pin_st;
  HIPCHK(hipMemcpyAsync(st, h->asm_status, (size_t)nprob * sizeof(int), hipMemcpyDeviceToHost, s));
  int* pin_its = h->pin_cnt + NVIEW * ASM_NCNT;
  if (h->profiling && c.pred_flops_per_it > 0.0) HIPCHK(hipMemcpyAsync(pin_its, h->pred_cnt + 1, 4, hipMemcpyDeviceToHost, s));
  if (c.defer_cnt) HIPCHK(hipMemcpyAsync(h->pin_cnt, h->view[0].counters, NVIEW * ASM_NCNT * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(stream_sync(s));
  if (c.defer_cnt) h->stats.asm_full_checks += ndone(h);
  if (h->profiling && c.pred_flops_per_it > 0.0) h->stats.asm_predict_flops += c.pred_flops_per_it * (double)*pin_its;
  HIPCHK(hipGetLastError());
  int ninvalid = 0;
  for (int p = 0; p < nprob; ++p) { if (st[p] == 3) fb.push_back(p); else if (st[p] != 0) ++ninvalid; }   // 2: rejected inputs
  h->stats.asm_solved += nprob - (int64_t)fb.size() - ninvalid;
  if (st_dev) HIPCHK(hipMemcpyAsync(st_dev, h->asm_status, (size_t)nprob * sizeof(int), hipMemcpyDeviceToDevice, s));
  return 0;
}

// What the pass could not finish (fb) is re-solved by the PDIP path (solve_segment) on a compacted copy (scratch owned by the
// handle: nothing to release on an error path) -- or, with opts.method == 2, reported as not certified.
int pdip_fallback(AsmCall& c, const std::vector<int>& fb, const double* x0_dev, int32_t* st_dev) {
  nnmpc_qp* h = c.h;
  hipStream_t s = c.s;
  const AsmDev& a = c.a;
  const int nprob = c.nprob;
  if (fb.empty()) { h->stats.problems += nprob; return 0; }
  if (h->opts.method == 2) {                           // asm only: report the rest as not certified
    int* st = h->pin_st;
    for (int p = 0; p < nprob; ++p) st[p] = st[p] == 3 ? NNMPC_ST_MAXITER : st[p];
    if (st_dev) HIPCHK(hipMemcpy(st_dev, st, (size_t)nprob * sizeof(int), hipMemcpyHostToDevice));
    h->stats.problems += nprob;
    return 0;
  }
  const int cntf = (int)fb.size();
  int* list = nullptr; double *x0c = nullptr, *lbc = nullptr, *ubc = nullptr, *uc = nullptr;
  uint32_t* actc = nullptr; int *stc = nullptr, *itc = nullptr;
  unsigned char* guessc = nullptr;
  DevRes& res = h->res;
  if (int rc = res.slot(nnmpc_qp::SC_FB_GUESS, &guessc, (size_t)cntf * h->n)) return rc;
  if (int rc = res.slot(nnmpc_qp::SC_FB_LIST, &list, cntf * sizeof(int))) return rc;
  if (int rc = res.slot(nnmpc_qp::SC_FB_X0, &x0c, (size_t)cntf * h->n_aug * 8)) return rc;
  if (int rc = res.slot(nnmpc_qp::SC_FB_LB, &lbc, (size_t)cntf * h->nu * 8)) return rc;
  if (int rc = res.slot(nnmpc_qp::SC_FB_UB, &ubc, (size_t)cntf * h->nu * 8)) return rc;
  if (int rc = res.slot(nnmpc_qp::SC_FB_U, &uc, (size_t)cntf * h->n * 8)) return rc;
  if (int rc = res.slot(nnmpc_qp::SC_FB_ACT, &actc, (size_t)cntf * h->words * 4)) return rc;
  if (int rc = res.slot(nnmpc_qp::SC_FB_ST, &stc, (size_t)cntf * 4)) return rc;
  if (int rc = res.slot(nnmpc_qp::SC_FB_IT, &itc, (size_t)cntf * 8)) return rc;
  int rc = 0;
  HIPCHK(hipMemcpy(list, fb.data(), cntf * sizeof(int), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(asm_gather_k, dim3(cntf), dim3(128), 0, s, x0c, lbc, ubc, x0_dev, a.lb, a.ub, list, cntf, h->n_aug, h->nu);
  // a problem whose set had settled but failed the check with P (inverse too inaccurate for its x) starts the polish
  // on that set; the others (not settled, too large, not positive definite) run the PDIP from scratch
  hipLaunchKernelGGL(asm_gather_guess_k, dim3(cntf), dim3(128), 0, s, guessc, h->asm_st, h->asm_state, list, cntf, h->n);
  for (int b0 = 0; b0 < cntf && !rc; b0 += h->seg_max) {
    const LayoutScope whole(h, h->n, h->n);            // the compacted copies hold whole sequences
    const int nb = std::min(h->seg_max, cntf - b0);
    rc = solve_segment(h, nb, x0c + (size_t)b0 * h->n_aug, lbc + (size_t)b0 * h->nu, ubc + (size_t)b0 * h->nu, guessc + (size_t)b0 * h->n,
                       uc + (size_t)b0 * h->n, actc + (size_t)b0 * h->words, stc + b0, itc + 2 * (size_t)b0);
  }
  if (!rc) {
    hipLaunchKernelGGL(asm_scatter_k, dim3(cntf), dim3(128), 0, s, a.u_out, a.act_out, st_dev, a.iters_out, uc, actc, stc, itc,
                       list, cntf, h->n, h->words, h->ldu, h->nout);
    HIPCHK(stream_sync(s));
  }
  h->stats.problems += nprob - cntf;   // solve_segment counted the fallback ones
  return rc;
}

// Shared-inverse active-set pass over one segment; problems it cannot finish are marked 3 in
// h->asm_status and re-solved by the PDIP path (solve_segment) on a compacted copy.
int solve_segment_asm(nnmpc_qp* h, int nprob, const double* x0_dev, const double* lb_dev, const double* ub_dev,
                      const unsigned char* guess_dev, double* u_dev, uint32_t* act_dev, int32_t* st_dev, int32_t* it_dev) {
  AsmCall c;
  AsmDev& a = c.a;
  const AsmSwitches& sw = asm_switches();
  hipStream_t s = h->stream;
  c.h = h; c.s = s; c.sw = &sw; c.nprob = nprob; c.segp = ((nprob + 127) / 128) * 128;
  hipLaunchKernelGGL(pad_x0_k, dim3(512), dim3(256), 0, s, h->x0_64, h->x0_32, x0_dev, nprob, h->n_aug, h->ka, c.segp);
  c.tail_only = h->opts.asm_tail_batch >= 0 && nprob <= std::min(std::min(h->asm_pool, 256), h->opts.asm_tail_batch ? h->opts.asm_tail_batch : 256);
  // x_unc = Kunc x0 -- for the leading columns only (the window the first sets are drawn from; extended should a round's
  // window outgrow it): beyond them x_unc is one K segment of the full-width pass's GEMM (qp_wide.h).  Calls that go to
  // the device tail from the start, and shapes the fused kernel's tiles do not fit, form all of it.  q = tq x0 is only
  // formed for the rows that need the full check with P.
  // Small problems -- Pinv fits the 4 MB L2 of an XCD (n <= 724: the CSTRs size, 540) -- run the whole iteration in one wave each
  // (qp_small.h); what that kernel hands back (sets beyond 64 bounds, problems still moving after its budget) carries on below.
  c.small = !env_no_small() && (size_t)h->np * h->np * 8 <= (4u << 20) && h->n <= ASM_SM_NMAX && h->np % 4 == 0;
  c.lazy = h->np % 128 == 0 && !sw.no_fused_wide && !sw.no_lazy_xunc && !c.tail_only && !c.small && (uint64_t)h->seg_max * h->ka * 8 < (1ull << 32);
  // (the window the first sets are drawn from: the leading eighth of the horizon, 512 columns at least -- a quarter until round 3;
  // the CDU batch settles inside 512 columns, a quarter is 1152: 0.4 ms of x_unc GEMM per step.  A bound x_unc violates further
  // out joins through the full-width pass every problem goes through.  Following the previous call's window instead made the
  // path of a call depend on the handle's history: other windows, other far-field factors, and for degenerate problems other sets)
  c.winit = std::min(h->n, std::max(512, ((h->n / 8 + 127) / 128) * 128));
  c.Wx = h->np;
  if (c.lazy) c.Wx = std::min(h->np, guess_dev ? 512 : ((c.winit + 127) / 128) * 128);
  {
    EvScope es(h, EV_GEMM, 2.0 * c.Wx * (double)h->ka * nprob);
    gemm64(h, h->asm_xunc, h->np, h->x0_64, h->ka, h->Kunc64, h->ka, c.segp, c.Wx, h->ka);
  }
  asm_args(c, lb_dev, ub_dev, guess_dev, u_dev, act_dev, it_dev);
  // LAM / LAMW are all zero between calls: every entry the multiplier kernels write is cleared again by
  // asm_update_k / asm_wide_k of the same round
  if (!guess_dev) HIPCHK(hipMemsetAsync(h->asm_st, 0, (size_t)nprob * h->n, s));   // bound states: asm_init_k writes the leading window only
  if (int rc = first_sets(c)) return rc;
  memset(h->pin_cnt, 0, NVIEW * ASM_NCNT * sizeof(int));
  HIPCHK(hipMemsetAsync(h->view[0].counters, 0, NVIEW * ASM_NCNT * sizeof(int), s));   // (all views' counters)
  if (c.small)
    if (int rc = small_pass(c)) return rc;
  c.defer_cnt = c.tail_only && !sw.trace;
  if (c.tail_only)
    if (int rc = tail_only_pass(c)) return rc;
  c.overlap_on = h->opts.asm_overlap >= 0 && h->view[1].rows > 0 && !env_overlap_off();
  // (as refine_later: only behind predicted first sets)
  c.carry_on = a.refine_later && a.pred_w && !c.tail_only && !env_carry_off();
  if (c.carry_on)
    if (int rc = h->res.slot(nnmpc_qp::SC_CARRY, &a.stash, (size_t)h->seg_max * ASM_MLDS * sizeof(double))) return rc;
  c.views3 = c.overlap_on && h->nview == NVIEW && !env_two_views();
  for (int v = 0; v < NVIEW; ++v) c.vW[v] = h->np;

  // ---- The pass beside the round.  A far-field full-width pass does not wait on the main stream: asm_wide_t_k (+ asm_wide_tnorm_k) and
  // asm_wide_gemm_k run on stream4 over the rows of the view the last round ran in (the pending view, c.pend; its rows and window:
  // c.vrows, c.vW), while the problems that did NOT settle in that round -- known since its asm_update_k -- are counted and, if they
  // fit, run their next round (or the device tail) on the main stream in the other, free view (rv): its own rows of LAM / XH, its own
  // counters and k-ranges.  Then the main stream waits for the pass and runs asm_wide_k (finish_passes).  Views swap roles from
  // iteration to iteration.  Two rules keep this free of races:
  //  (1) asm_wide_k is the only kernel of the pass that writes `state` (ASM_WIDE -> RUN / CERT / DONE), and asm_count_k, the bins,
  //      asm_update_k and asm_taillist_k scan `state` over all problems: finish_passes runs on the main stream after everything the
  //      round enqueued there and on its side streams (their joins come before the round's GEMMs: launch_multipliers).  Problems it
  //      sends back to ASM_RUN are found by the next iteration's count, which is why the loop goes on after an overlapped tail.
  //  (2) asm_wide_t_k / asm_wide_gemm_k write st / wflag / u_out / T only for rows with rowprob >= 0: problems in state ASM_WIDE, which
  //      no kernel of the round touches (it works on ASM_RUN problems); the far-field form reads no x_unc beyond the window, so an
  //      x_unc extension or the tail's gathered x_unc rows (extend_xunc: c.Wx, c.a.Wx) do not collide with it.  The dense, lazy and
  //      plain-GEMM forms of the pass keep the serial order (launch_pass leaves pl.inflight false).
  // The size-class lists, ranks and chunk totals (binlist, biglist, lrank, ctot) live from a round's bins to its multiplier kernels,
  // all ordered on the main stream, and the pass reads none of them: all views share them.
  // ---- A second iteration beside the same pass (the third view).  After a round that ran beside a pass the loop does not join that
  // pass at once: the round's own pass, if it has one, is launched on stream4 BEHIND the first (stream order serialises them; each has
  // its completion event, h->ev_wide[view]), the problems still running are counted in the view neither pass holds and run their
  // next round or the tail there, and only then are the passes finished, in launch order (finish_passes).  Nothing in that iteration
  // needs the first pass's outcome: its problems are ASM_RUN since the round's asm_update_k, the passes' are ASM_WIDE, and whatever an
  // asm_wide_k sends back is found by the count after it.  Both rules hold as they stand, for either pass.  At most one such
  // iteration per first pass (`chained`), and only behind a pass of the far-field form; after an overlapped tail nothing runs any
  // more, so the loop joins at once as before.  NNMPC_VIEWS=2 (read per call) restores the order of two views.
  const int round_cap = 2 * a.max_rounds + 2;
  int rounds = 0;
  PassFifo fly;
  bool chained = false;                                  // this iteration is the second one beside fly.pl[0]
  for (; !c.tail_only && rounds < round_cap; ++rounds) {
    const int pv = c.pend;
    if (pv >= 0) {
      PassLaunch& pl = fly.pl[fly.n];
      pl = PassLaunch{a, -1, false, pv, WideStat{false, 0, 0, 0, 0, 0.0}};
      if (int rc = launch_pass(c, pv, pl, fly.n > 0)) return rc;
      if (pl.inflight) fly.n += 1;
    }
    if (!a.pred_w) a.refine_later = 0;                   // (only behind predicted first sets: from other starts the f32 rounds are many and their sets still move)
    a.refine = a.refine_later && rounds >= 1;            // round 0 stays the plain f32 screen
    // ... which keeps the corrected multipliers of the sets it leaves as they are: round 1 copies them (a flag asm_update_k raised
    // in round 0 is read by round 1's count and bins, cleared by its asm_carry_copy, and by nobody after that)
    a.carry = c.carry_on ? (rounds == 0 ? 1 : (rounds == 1 ? 2 : 0)) : 0;
    a.kref = c.kprev;
    // the round's view: beside passes the first one none of them occupies, view 0 otherwise
    int rv = 0;
    while (fly.n && fly.holds(rv)) ++rv;
    if (rv >= h->nview) { set_error("solve_segment_asm: no free row space beside %d passes", fly.n); return NNMPC_EINVAL; }
    int n64 = 0, n32 = 0, nrun = 0;
    const int* cnt = nullptr;
    for (bool recount = false;; recount = true) {
      if (int rc = count_round(c, rv, recount)) return rc;
      cnt = h->pin_cnt + rv * ASM_NCNT;
      n64 = cnt[ASM_CNT_ROWS64]; n32 = cnt[ASM_CNT_ROWS32]; nrun = n64 + n32;   // solved in fp64 / f32 this round
      if (!fly.n || nrun <= h->view[rv].rows) break;
      // more problems still running than the free view has rows (the early rounds of a call without predicted sets): the count was
      // hidden behind the pass but is of no use -- finish the passes and count again, in view 0, as the serial order would have
      if (int rc = finish_passes(c, fly)) return rc;
      chained = false;
      rv = 0;
    }
    const int beside = fly.n;                            // passes this iteration runs beside
    c.kprev = cnt[ASM_CNT_LAST];
    if (sw.trace) trace_round(rounds, beside, cnt);
    if (nrun == 0) {
      if (!beside) break;
      // nothing left to run beside the passes; asm_wide_k may still send problems back: the next count decides (this was no round)
      if (int rc = finish_passes(c, fly)) return rc;
      chained = false;
      --rounds;
      continue;
    }
    if (beside) {
      // (a pass is counted once, by the first iteration that runs beside it: the first pass of a chain was counted by its round)
      h->stats.asm_overlapped_passes += chained ? beside - 1 : 1;
      h->stats.asm_shared_passes += chained;
    }
    if (nrun <= std::min(h->asm_pool, sw.tail_max) && (rounds >= (a.pred_w ? 2 : 6) || c.small)) {
      if (int rc = run_tail(c, rv, nrun, rounds, beside > 0)) return rc;
      if (!beside) {
        rounds = 0;                                       // (regular exit: the counters just read are final)
        break;
      }
      a.Wx = c.Wx;                                        // (x_unc beyond Wx exists for the tail's problems only)
      if (int rc = finish_passes(c, fly)) return rc;
      chained = false;
      continue;                                           // (the next count ends the loop, or finds what asm_wide_k sent back)
    }
    h->stats.asm_rounds += 1;
    h->stats.asm_carried += cnt[ASM_CNT_CARRY];
    // column window of this round: past the last active bound of any running problem plus one stage; a
    // problem that settles inside it gets one full-width pass (asm_wide_k) at the start of the next round
    a.W = std::min(h->np, ((cnt[ASM_CNT_LAST] + 1 + h->nu + 127) / 128) * 128);
    if (a.W > c.Wx) {
      // a set reaches beyond the columns x_unc was formed for (a bound the full-width pass found violated out there): extend
      EvScope es(h, EV_GEMM, 2.0 * (a.W - c.Wx) * (double)h->ka * nprob);
      extend_xunc(c, a.W, c.segp, false);
    }
    if (int rc = launch_multipliers(c, cnt, beside > 0)) return rc;
    if (sw.trace && a.carry)
      if (int rc = trace_carry(c, rounds, cnt)) return rc;
    if (int rc = window_gemms_and_update(c, rv, n64, n32, cnt)) return rc;
    c.vW[rv] = a.W;
    c.vrows[rv] = a.W < h->n ? n64 : 0;                  // fp64 rows of this round: the problems that settled in them await the full-width check
    c.pend = c.vrows[rv] ? rv : -1;
    if (beside) {
      // once per first pass: go round again without joining it, if the third view is there and this round's pass can queue behind it
      int c0 = 0, fused_c0 = -1;
      if (!chained && beside == 1 && c.views3 && (c.pend < 0 || pass_form(c, c.pend, &c0, &fused_c0))) {
        chained = true;
        continue;
      }
      if (int rc = finish_passes(c, fly)) return rc;
      chained = false;
    }
  }
  if (fly.n)                                             // (the round cap ended a chain)
    if (int rc = finish_passes(c, fly)) return rc;
  std::vector<int> fb;
  if (int rc = certify_and_collect(c, rounds >= round_cap, st_dev, fb)) return rc;
  return pdip_fallback(c, fb, x0_dev, st_dev);
}

// Bound multipliers of nprob delivered rows (qp_mult.h), enqueued on the handle's stream; device pointers.
int launch_mult(nnmpc_qp* h, int nprob, const double* x0_dev, const double* u_dev, const uint32_t* act_dev, const int32_t* st_dev,
                double* mult_dev) {
  MultArgs m;
  m.P64 = h->P64; m.tq64 = h->tq64; m.x0 = x0_dev; m.u = u_dev; m.active = act_dev; m.status = st_dev; m.mult = mult_dev;
  m.n = h->n; m.np = h->np; m.nu = h->nu; m.n_aug = h->n_aug; m.ka = h->ka; m.words = h->words;
  EvScope es(h, EV_MULT, 0.0);
  hipLaunchKernelGGL(asm_mult_k, dim3(nprob), dim3(MULT_THREADS), 0, h->stream, m);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // namespace

hipStream_t nnmpc_qp_stream_internal(nnmpc_qp* h) { return h->stream; }

extern "C" {

int nnmpc_qp_create(nnmpc_qp** out, int32_t n, int32_t nu, int32_t n_aug, const double* P,
                    const double* tq, const double* Kunc, const nnmpc_qp_opts* opts) {
  if (!out || !P || !tq || n <= 0 || nu <= 0 || nu > 256 || n_aug <= 0 || n % nu != 0) {
    set_error("nnmpc_qp_create: bad arguments (n=%d nu=%d n_aug=%d)", n, nu, n_aug);
    return NNMPC_EINVAL;
  }
  GUARD_BEGIN
  if (int rc = check_device(__func__)) return rc;
  Building<nnmpc_qp, nnmpc_qp_destroy> guard(new nnmpc_qp());   // released into *out at the end; destroyed on any other way out
  nnmpc_qp* h = guard.get();
  DevRes& res = h->res;
  memset(&h->stats, 0, sizeof(h->stats));
  memset(&h->d, 0, sizeof(h->d));
  h->profiling = false; h->ev_used = 0; h->have_inverse = false;
  h->ldu = n; h->nout = n;
  if (opts) h->opts = *opts; else memset(&h->opts, 0, sizeof(h->opts));
  nnmpc_qp_opts& o = h->opts;
  if (o.max_batch <= 0) o.max_batch = 1024;
  if (o.nb == 0) o.nb = (n <= 1024) ? 64 : 128;
  if (o.nb != 64 && o.nb != 128) { set_error("nb must be 64 or 128"); return NNMPC_EINVAL; }
  if (o.max_ipm_iters <= 0) o.max_ipm_iters = 40;
  if (o.max_polish_rounds <= 0) o.max_polish_rounds = 150;
  if (o.max_refine <= 0) o.max_refine = 60;
  if (o.max_rounds <= 0) o.max_rounds = 1000;
  if (o.sub_steps <= 0) o.sub_steps = 8;
  if (o.stale_max_changes == 0) o.stale_max_changes = 4;   // < 0 disables factor reuse
  if (o.stale_cg_limit <= 0) o.stale_cg_limit = 16;
  if (o.asm_max_active <= 0) o.asm_max_active = 768;
  if (o.asm_max_active > 768) o.asm_max_active = 768;
  o.asm_max_active = std::max(16, (o.asm_max_active / 16) * 16);
  // the device tail (asm_tail_k) gets 50 000 iterations unless the caller set a budget: Murty's rule is finite but slow on dense
  // Hessians with cond >= 1e5 and half the bounds active -- scripts/stress_asm.py, seeds 1 and 3: 130 and 166 of ~1600 problems
  // unfinished after 200 iterations, 27 and 1 after 4000, none after 30 000 (a straggler then holds one workgroup for ~1 s; the
  // problems of the reference's regime settle within 40 iterations and never see the difference)
  h->asm_tail_budget = o.asm_max_rounds <= 0 ? 50000 : o.asm_max_rounds;
  if (o.asm_max_rounds <= 0) o.asm_max_rounds = 200;
  if (o.asm_predict_iters > PRED_MAXIT) o.asm_predict_iters = PRED_MAXIT;   // (0: adaptive, 8 .. PRED_MAXIT by workgroup)
  if (o.sub_steps < 2) o.sub_steps = 2;
  if (o.ipm_tol <= 0.f) o.ipm_tol = 1e-2f;
  if (o.refine_tol <= 0.0) o.refine_tol = 1e-10;
  if (o.bound_tol <= 0.0) o.bound_tol = 1e-9;
  HIPCHK(hipGetDevice(&h->device));
  res.device = h->device;
  h->n = n; h->nu = nu; h->n_aug = n_aug;
  h->NB = o.nb;
  h->np = ((n + h->NB - 1) / h->NB) * h->NB;
  h->T = h->np / h->NB;
  h->tiles = h->T * (h->T + 1) / 2;
  h->ka = ((n_aug + 31) / 32) * 32;
  h->slots = ((o.max_batch + 127) / 128) * 128;
  h->words = (2 * n + 31) / 32;
  h->have_kunc = Kunc != nullptr;
  if ((size_t)(h->np + 5 * h->NB) * 4 > 96 * 1024) { set_error("n too large for the LDS-resident solve vector"); return NNMPC_EINVAL; }
  for (hipStream_t* st : {&h->stream, &h->stream2, &h->stream3, &h->stream4})
    if (int rc = res.stream(st)) return rc;
  for (hipEvent_t* ev : {&h->ev_fork, &h->ev_join3, &h->ev_join4, &h->ev_join, &h->ev_wfork, &h->ev_wide[0], &h->ev_wide[1], &h->ev_wide[2]})
    if (int rc = res.event(ev, hipEventDisableTiming)) return rc;
  HIPCHK(hipFuncSetAttribute((const void*)asm_lambda_reg_k, hipFuncAttributeMaxDynamicSharedMemorySize, ASM_REG_LDS));
  HIPCHK(hipFuncSetAttribute((const void*)asm_lambda_reg32_k, hipFuncAttributeMaxDynamicSharedMemorySize, ASM_REG32_LDS));
  HIPCHK(hipFuncSetAttribute((const void*)asm_tail_k, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
  HIPCHK(hipFuncSetAttribute((const void*)asm_lambda_reg32b_k, hipFuncAttributeMaxDynamicSharedMemorySize, ASM_REG32B_LDS));
  HIPCHK(hipFuncSetAttribute((const void*)gemm_nt_f64_t128_k, hipFuncAttributeMaxDynamicSharedMemorySize, G64_LDS));
  HIPCHK(hipFuncSetAttribute((const void*)asm_wide_gemm_k<WIDE_XUNC>, hipFuncAttributeMaxDynamicSharedMemorySize, G64_LDS));
  HIPCHK(hipFuncSetAttribute((const void*)asm_wide_gemm_k<WIDE_LAZY>, hipFuncAttributeMaxDynamicSharedMemorySize, G64_LDS));
  HIPCHK(hipFuncSetAttribute((const void*)asm_wide_gemm_k<WIDE_FAR>, hipFuncAttributeMaxDynamicSharedMemorySize, G64_LDS));
  HIPCHK(hipFuncSetAttribute((const void*)asm_wide_t_k, hipFuncAttributeMaxDynamicSharedMemorySize, G64_LDS));
  HIPCHK(hipFuncSetAttribute((const void*)asm_small_k<9, 1, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, ASM_SMALL9_LDS_MAX));
  HIPCHK(hipFuncSetAttribute((const void*)gemm_nt_f32_kdyn_k<128>, hipFuncAttributeMaxDynamicSharedMemorySize, TileCfg<128>::LDS_FLOATS * 4));
  HIPCHK(hipFuncSetAttribute((const void*)sens_k<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sens_lds_bytes<false>()));
  HIPCHK(hipFuncSetAttribute((const void*)sens_k<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sens_lds_bytes<true>()));
  HIPCHK(hipFuncSetAttribute((const void*)adj_k<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sens_lds_bytes<false>()));
  HIPCHK(hipFuncSetAttribute((const void*)adj_k<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sens_lds_bytes<true>()));
  if (int rc = set_lds_attrs<128>()) return rc;
  if (int rc = set_lds_attrs<64>()) return rc;

  const int np = h->np, NB = h->NB, ka = h->ka, S = h->slots;
  const size_t nb2 = (size_t)NB * NB;
#define A_(ptr, cnt) if (int rc = res.alloc(&(ptr), (size_t)(cnt))) return rc
  A_(h->Pt, h->tiles * nb2); A_(h->P32, (size_t)np * np); A_(h->P64, (size_t)np * np);
  A_(h->tq64, (size_t)np * ka); A_(h->Kunc32, (size_t)np * ka); A_(h->pdiag, np);
  A_(h->L, (size_t)S * h->tiles * nb2); A_(h->Y, (size_t)S * h->T * nb2); A_(h->Dacc, (size_t)S * h->T * nb2); A_(h->trsv_count, 1);
  QpDev& d = h->d;
  const size_t V = (size_t)S * np;
  A_(d.u, V); A_(d.zu, V); A_(d.zl, V); A_(d.lbv, V); A_(d.ubv, V); A_(d.q, V); A_(d.PU, V);
  A_(d.rd, V); A_(d.rhs, V); A_(d.sol, V); A_(d.dua, V); A_(d.dvec, V); A_(d.mask, V); A_(d.uunc, V);
  A_(d.x, V); A_(d.q64, V); A_(d.PX, V); A_(d.r64, V); A_(d.p64, V); A_(d.v64, V); A_(d.st, V);
  A_(d.phase, S); A_(d.f_factor, S); A_(d.f_solve, S); A_(d.istep, S); A_(d.ipm_it, S);
  A_(d.nfac, S); A_(d.prounds, S); A_(d.pninf, S); A_(d.pgrace, S); A_(d.ptie, S); A_(d.rcnt, S); A_(d.psub, S); A_(d.fail, S); A_(d.stale, S); A_(d.rz, S);
  A_(d.mu, S); A_(d.gap, S); A_(d.smu, S); A_(d.qscale, S); A_(d.counters, 8);
  {
    // segment size: as many problems as a quarter of the free HBM allows (per problem: q f64, warm start f32 and the
    // six f64 rows of the active-set pass, its set list and bound states).  Large segments amortise the thinly
    // populated last rounds of the active-set pass.
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)12e9;
    long long cap = (long long)(0.25 * (double)free_b / (12.0 * np + 88.0 * np + n + 4.0 * o.asm_max_active + 64.0));
    if (o.seg_max > 0) cap = std::min<long long>(cap, o.seg_max);
    cap = std::max<long long>(cap, S);
    cap = std::min<long long>(cap, 1 << 20);
    h->seg_max = (int)((cap / 128) * 128);
  }
  const size_t G = h->seg_max;
  A_(h->x0_64, G * ka); A_(h->x0_32, G * ka);
  A_(h->q64_all, G * np); A_(h->uunc_all, G * np);
  A_(h->lb_d, G * nu); A_(h->ub_d, G * nu);
  A_(h->in_stage, G * n_aug);
  if (int rc = res.pinned_alloc(&h->pin_cnt, nnmpc_qp::ASM_NVIEW * ASM_NCNT + 4)) return rc;
  if (int rc = res.pinned_alloc(&h->pin_st, G)) return rc;
  A_(d.lb64, (size_t)S * nu); A_(d.ub64, (size_t)S * nu);
  A_(d.slot_prob, S); A_(d.age, S); A_(d.next_prob, 1);
  // workgroups of the large-set kernel in flight (each with its tile slab in HBM / L2): four per CU for bulk batches --
  // the kernel is a latency chain (barriers, tiles in global memory), occupancy is what hides it
  h->asm_pool = h->seg_max >= 4096 ? (asm_switches().tail_max > 1024 ? 2048 : 1024) : 256;
  nnmpc_qp::AsmView& v0 = h->view[0];
  A_(h->H64, (size_t)np * np); A_(h->Kunc64, (size_t)np * ka); A_(h->H32, (size_t)np * np);
  A_(h->asm_xunc, G * np); A_(h->asm_x, G * np); A_(v0.lam, G * np); A_(v0.xh, G * np);
  A_(v0.xhw, (G + 256) * np); A_(v0.rowprob, G + 256); A_(h->asm_wflag, G); A_(h->asm_wmark, G);
  A_(v0.tnorm, G + 128 * (ASM_NKG + 1)); A_(v0.tslack, G + 128 * (ASM_NKG + 1));
  A_(h->asm_st, G * n); A_(h->asm_state, G); A_(h->asm_rounds, G); A_(v0.counters, nnmpc_qp::ASM_NVIEW * ASM_NCNT);
  A_(h->asm_biglist, G); A_(h->asm_status, G); A_(h->asm_binlist, (size_t)(ASM_NLIST + 4) * G);
  A_(h->asm_idxg, G * o.asm_max_active); A_(h->asm_mg, G); A_(h->asm_row, G); A_(h->asm_lrank, G); A_(h->asm_ctot, ((G + 1023) / 1024) * ASM_NSCAN); A_(h->asm_prec, G); A_(h->asm_redo, G); A_(h->asm_rowk, G); A_(h->asm_cflag, G); A_(h->asm_carrylist, G); A_(v0.lam32, G * np); A_(v0.xh32, G * np); A_(h->asm_alpha, G); A_(h->asm_ninf, G); A_(h->asm_hi, G); A_(v0.kblk, 2 * (G / 64 + 2)); A_(h->asm_work, 3 * G);
  v0.rows = (int)G;
  A_(h->asm_scratch, (size_t)h->asm_pool * ((size_t)(o.asm_max_active / 16) * (o.asm_max_active / 16 + 1) / 2 * ASM_TS));
  {
    // the second row space: a thirty-second of the segment, 1024 rows at least (the CDU batch of 100 000 at sx = 2 leaves ~1 300
    // problems running after the round most sets settle in: 3 200 rows, 0.47 GB at np = 4608).  Its k-range array is as long as view
    // 0's: asm_bins_b_k writes the entry of every row it hands out, also in a round that turns out not to fit these rows.
    // (NNMPC_OVERLAP_ROWS: tests only -- a row count that forces the rounds back into view 0)
    long long R = env_overlap_rows(std::max<long long>(1024, ((long long)G / 32 + 127) / 128 * 128));
    R = std::min<long long>(R, (long long)G);
    if (o.asm_overlap >= 0 && R > 0) {
      nnmpc_qp::AsmView& v1 = h->view[1];
      const size_t Rr = (size_t)R;
      A_(v1.lam, Rr * np); A_(v1.xh, Rr * np); A_(v1.xhw, (Rr + 256) * np); A_(v1.lam32, Rr * np); A_(v1.xh32, Rr * np);
      A_(v1.tnorm, Rr + 128 * (ASM_NKG + 1)); A_(v1.tslack, Rr + 128 * (ASM_NKG + 1)); A_(v1.rowprob, Rr + 256); A_(v1.kblk, 2 * (G / 64 + 2));
      v1.counters = v0.counters + ASM_NCNT;
      v1.rows = (int)R;
      h->nview = 2;
      // the third row space, sized like the second (another 0.47 GB at the CDU segment): the iteration after the round beside a
      // pass runs in it, beside the same pass.  A handle that cannot have it works with two views.
      nnmpc_qp::AsmView v2;
      const bool ok = !res.alloc(&v2.lam, Rr * np) && !res.alloc(&v2.xh, Rr * np) && !res.alloc(&v2.xhw, (Rr + 256) * np) &&
                      !res.alloc(&v2.lam32, Rr * np) && !res.alloc(&v2.xh32, Rr * np) &&
                      !res.alloc(&v2.tnorm, Rr + 128 * (ASM_NKG + 1)) && !res.alloc(&v2.tslack, Rr + 128 * (ASM_NKG + 1)) &&
                      !res.alloc(&v2.rowprob, Rr + 256) && !res.alloc(&v2.kblk, 2 * (G / 64 + 2));
      if (ok) {
        v2.counters = v0.counters + 2 * ASM_NCNT;
        v2.rows = (int)R;
        h->view[2] = v2;
        h->nview = 3;
      } else {
        for (void* p : {(void*)v2.lam, (void*)v2.xh, (void*)v2.xhw, (void*)v2.lam32, (void*)v2.xh32, (void*)v2.tnorm, (void*)v2.tslack,
                        (void*)v2.rowprob, (void*)v2.kblk})
          (void)res.give_back(p);
        (void)hipGetLastError();                    // (the failed hipMalloc is not an error of this handle)
      }
    }
  }
  static_assert(nnmpc_qp::ASM_NVIEW == 3, "the views made here, their events above");
#undef A_
  d.n = n; d.np = np; d.nu = nu; d.slots = S; d.words = h->words;
  d.max_ipm = o.max_ipm_iters; d.max_polish = o.max_polish_rounds; d.max_refine = o.max_refine;
  d.max_rounds = o.max_rounds; d.stale_max_changes = o.stale_max_changes; d.stale_cg_limit = o.stale_cg_limit;
  d.ipm_tol = o.ipm_tol; d.refine_tol = o.refine_tol; d.bound_tol = o.bound_tol; d.stat_tol = 1e-8;

  // host-side packing of the shared matrices (one-time setup)
  std::vector<float> pt(h->tiles * nb2, 0.f), p32((size_t)np * np, 0.f), k32((size_t)np * ka, 0.f), pdg(np, 1.f);
  std::vector<double> p64((size_t)np * np, 0.0), t64((size_t)np * ka, 0.0);
  {
    std::vector<double> dg(n);
    for (int r = 0; r < n; ++r) dg[r] = P[(size_t)r * n + r];
    std::nth_element(dg.begin(), dg.begin() + n / 2, dg.end());
    h->pscale = dg[n / 2];
    if (!(h->pscale > 0.0)) { set_error("P has a non-positive diagonal"); return NNMPC_EINVAL; }
  }
  const double ips = 1.0 / h->pscale;
  float pdmax = 0.f;
  for (int r = 0; r < n; ++r) {
    pdg[r] = (float)(P[(size_t)r * n + r] * ips);
    pdmax = std::max(pdmax, pdg[r]);
    for (int c = 0; c <= r; ++c) {
      const double v = P[(size_t)r * n + c];  // lower triangle is authoritative
      p64[(size_t)r * np + c] = v; p64[(size_t)c * np + r] = v;
      p32[(size_t)r * np + c] = (float)(v * ips); p32[(size_t)c * np + r] = (float)(v * ips);
    }
  }
  d.pscale = h->pscale;
  for (int r = 0; r < n; ++r) {
    double rs = 0.0;
    for (int c = 0; c < n; ++c) rs += std::fabs(p64[(size_t)r * np + c]);
    h->p_inf = std::max(h->p_inf, rs);
  }
  d.delta = 16.f * 5.96e-8f * pdmax;   // keeps the f32 Cholesky positive for cond(P) >~ 1e7
  d.pdiag = h->pdiag;
  for (int i = 0; i < h->T; ++i)
    for (int j = 0; j <= i; ++j) {
      float* t = pt.data() + ((size_t)i * (i + 1) / 2 + j) * nb2;
      for (int r = 0; r < NB; ++r)
        for (int c = 0; c < NB; ++c) {
          const int gr = i * NB + r, gc = j * NB + c;
          float v = 0.f;
          if (gr < n && gc < n) v = (float)((gc <= gr ? P[(size_t)gr * n + gc] : P[(size_t)gc * n + gr]) * ips);
          else if (gr == gc) v = 1.f;
          t[(size_t)r * NB + c] = v;
        }
    }
  h->tqmax = 0.0;
  for (int r = 0; r < n; ++r)
    for (int k = 0; k < n_aug; ++k) {
      t64[(size_t)r * ka + k] = tq[(size_t)r * n_aug + k];
      h->tqmax = std::max(h->tqmax, std::fabs(tq[(size_t)r * n_aug + k]));
      if (Kunc) k32[(size_t)r * ka + k] = (float)Kunc[(size_t)r * n_aug + k];
    }
  HIPCHK(hipMemcpy(h->Pt, pt.data(), pt.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->P32, p32.data(), p32.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->P64, p64.data(), p64.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->tq64, t64.data(), t64.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->Kunc32, k32.data(), k32.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->pdiag, pdg.data(), pdg.size() * 4, hipMemcpyHostToDevice));
  *out = guard.release();
  return NNMPC_OK;
  GUARD_END
}

int nnmpc_qp_destroy(nnmpc_qp* h) {
  if (!h) return NNMPC_OK;
  h->res.release();
  delete h;
  return NNMPC_OK;
}

int nnmpc_qp_set_inverse(nnmpc_qp* h, const double* Hinv, const double* Kunc) {
  if (!h || !Hinv || !Kunc) { set_error("nnmpc_qp_set_inverse: bad arguments"); return NNMPC_EINVAL; }
  GUARD_BEGIN
  HIPCHK(hipSetDevice(h->device));
  const int n = h->n, np = h->np, ka = h->ka, n_aug = h->n_aug;
  if ((uint64_t)np * np * 8 >= (1ull << 32)) {            // the multiplier kernels address Pinv with 32-bit byte offsets
    set_error("nnmpc_qp_set_inverse: n = %d is too large for the active-set pass (n < 23168)", n);
    return NNMPC_EINVAL;
  }
  // From here on the device copies of the previous pair are overwritten: the handle has no inverse until this pair has passed the
  // check below (a refused call leaves it to the PDIP path), and what was derived from the previous pair goes with it -- the
  // far-field factors and their verified error (their windows are asked for again once the new pair is in), the predictor images.
  HIPCHK(stream_sync(h->stream));
  h->have_inverse = false;
  h->kunct_ok = false;                                      // (nnmpc_qp_adjoint builds the accepted pair's image when it first needs it)
  h->res.drop_slot(nnmpc_qp::SC_A_KT);
  h->pred[0].L = h->pred[1].L = 0.0;
  std::vector<int> refactor;
  for (auto& g : h->far) {
    for (void* p : {(void*)g.U, (void*)g.Vx, (void*)g.Vl, (void*)g.cu, (void*)g.kt}) h->res.give_back(p);
    refactor.push_back(g.W);
  }
  h->far.clear();
  std::vector<double> hh((size_t)np * np, 0.0), kk((size_t)np * ka, 0.0);
  for (int r = 0; r < n; ++r) {
    for (int c = 0; c < n; ++c) hh[(size_t)r * np + c] = 0.5 * (Hinv[(size_t)r * n + c] + Hinv[(size_t)c * n + r]);
    for (int k = 0; k < n_aug; ++k) kk[(size_t)r * ka + k] = Kunc[(size_t)r * n_aug + k];
  }
  HIPCHK(hipMemcpy(h->H64, hh.data(), hh.size() * 8, hipMemcpyHostToDevice));
  {
    std::vector<float> h32(hh.size());
    for (size_t i = 0; i < hh.size(); ++i) h32[i] = (float)hh[i];
    HIPCHK(hipMemcpy(h->H32, h32.data(), h32.size() * 4, hipMemcpyHostToDevice));
  }
  HIPCHK(hipMemcpy(h->Kunc64, kk.data(), kk.size() * 8, hipMemcpyHostToDevice));
  // ---- first-set predictor (qp_predict.h): the 512-column window, and the 1024-column one for batches whose sets reach further
  h->pred[0].L = h->pred[1].L = 0.0;
  if (h->nu <= 64 && h->nu >= 4 && h->opts.asm_predict_iters >= 0) {
    if (np >= PRED_W && n >= PRED_W) {
      const int rc = build_predictor<4>(h, hh, np, h->pred[0]);
      if (rc) return rc;
      if (!h->pred_cnt) { const int rc2 = h->res.alloc(&h->pred_cnt, 4); if (rc2) return rc2; }
      HIPCHK(hipFuncSetAttribute((const void*)asm_predict_k<4, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, pred_lds_bytes<4, 4>(h->nu)));
      HIPCHK(hipFuncSetAttribute((const void*)asm_predict_k<4, 2, false>, hipFuncAttributeMaxDynamicSharedMemorySize, pred_lds_bytes<4, 2>(h->nu)));
    }
    if (np >= PRED_W2 && n >= PRED_W2 && h->pred[0].L > 0.0 && h->nu % 4 == 0) {
      const int rc = build_predictor<8>(h, hh, np, h->pred[1]);
      if (rc) return rc;
      HIPCHK(hipFuncSetAttribute((const void*)asm_predict_k<8, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, pred_lds_bytes<8, 2>(h->nu)));
    }
  }
  // ---- verify the inverse once, on the device copies the solves will use:
  //      E2 = P Pinv - I,  E1 = P Kunc + tq;  their maxima feed the per-problem certificate
  {
    const int kap = ((n_aug + 63) / 64) * 64;
    // tmp holds P Pinv (np x np), then P Kunc (np x kap): kap exceeds np when the horizon is short beside the state (n < n_aug)
    const size_t ntmp = (size_t)np * std::max(np, kap);
    std::vector<double> ktr((size_t)kap * np, 0.0);
    for (int r = 0; r < n; ++r)
      for (int k = 0; k < n_aug; ++k) ktr[(size_t)k * np + r] = Kunc[(size_t)r * n_aug + k];
    DevRes work;                                            // the two temporaries: freed on every way out of this block
    work.device = h->device;
    double *tmp = nullptr, *kt = nullptr;
    if (int rc = work.alloc(&tmp, ntmp)) return rc;
    if (int rc = work.upload(&kt, ktr.data(), ktr.size())) return rc;
    gemm64(h, tmp, np, h->P64, np, h->H64, np, np, np, np);                 // P Pinv (Pinv symmetric)
    HIPCHK(stream_sync(h->stream));
    std::vector<double> c(ntmp);
    HIPCHK(hipMemcpy(c.data(), tmp, (size_t)np * np * 8, hipMemcpyDeviceToHost));
    double e2 = 0.0;
    for (int r = 0; r < n; ++r)
      for (int cc = 0; cc < n; ++cc) e2 = std::max(e2, std::fabs(c[(size_t)r * np + cc] - (r == cc ? 1.0 : 0.0)));
    gemm64(h, tmp, kap, h->P64, np, kt, np, np, kap, np);                   // P Kunc  -> [np][kap]
    HIPCHK(stream_sync(h->stream));
    HIPCHK(hipMemcpy(c.data(), tmp, (size_t)np * kap * 8, hipMemcpyDeviceToHost));
    std::vector<double> tqh((size_t)np * ka);
    HIPCHK(hipMemcpy(tqh.data(), h->tq64, tqh.size() * 8, hipMemcpyDeviceToHost));
    double e1 = 0.0;
    for (int r = 0; r < n; ++r)
      for (int k = 0; k < n_aug; ++k) e1 = std::max(e1, std::fabs(c[(size_t)r * kap + k] + tqh[(size_t)r * ka + k]));
    h->asm_e1max = e1; h->asm_e2max = e2;
    if (!(e2 < 1e-6) || !(e1 == e1)) {
      set_error("nnmpc_qp_set_inverse: |P Pinv - I|_max = %.3e: the supplied inverse is not usable", e2);
      h->pred[0].L = h->pred[1].L = 0.0;                    // (images of the refused pair)
      return NNMPC_EINVAL;
    }
  }
  for (int W : refactor)
    if (h->far_missing.size() < 16 && std::find(h->far_missing.begin(), h->far_missing.end(), W) == h->far_missing.end()) h->far_missing.push_back(W);
  h->have_inverse = true;
  return NNMPC_OK;
  GUARD_END
}

int nnmpc_qp_set_farfield(nnmpc_qp* h, int32_t W, int32_t r, const double* U, const double* Vx, const double* Vl) {
  if (!h || !U || !Vx || !Vl || r <= 0) { set_error("nnmpc_qp_set_farfield: bad arguments"); return NNMPC_EINVAL; }
  if (!h->have_inverse) { set_error("nnmpc_qp_set_farfield: needs nnmpc_qp_set_inverse first"); return NNMPC_EINVAL; }
  GUARD_BEGIN
  HIPCHK(hipSetDevice(h->device));
  const int n = h->n, np = h->np, ka = h->ka, n_aug = h->n_aug;
  const int rp = ((r + 127) / 128) * 128;
  if (W <= 0 || W % 128 != 0 || W >= n || np % 128 != 0) { set_error("nnmpc_qp_set_farfield: W = %d must be a multiple of 128 below n = %d (padded %d)", W, n, np); return NNMPC_EINVAL; }
  // the factored form costs 2 rp (ka + W + columns beyond W) flops per problem, the dense form 2 (ka + W)(columns beyond W): refuse
  // factors that do not pay (a generic Hessian's far block has full rank; the MPC structure is what makes it ~Nx)
  if ((double)rp * (ka + W + (np - W)) > 0.8 * (double)(ka + W) * (np - W)) {
    set_error("nnmpc_qp_set_farfield: rank %d does not pay against the dense form at W = %d (n = %d, n_aug = %d)", r, W, n, n_aug);
    return NNMPC_EINVAL;
  }
  if (rp > np) { set_error("nnmpc_qp_set_farfield: rank %d too large for the workspace", r); return NNMPC_EINVAL; }
  const int nf = np - W;                                  // rows of the far block (padding rows: zero)
  std::vector<double> u((size_t)nf * rp, 0.0), vx((size_t)rp * ka, 0.0), vl((size_t)rp * W, 0.0), cu(nf / 128, 0.0);
  for (int j = 0; j < n - W; ++j)
    for (int i = 0; i < r; ++i) u[(size_t)j * rp + i] = U[(size_t)j * r + i];
  for (int i = 0; i < r; ++i) {
    for (int k = 0; k < n_aug; ++k) vx[(size_t)i * ka + k] = Vx[(size_t)i * n_aug + k];
    for (int k = 0; k < W; ++k) vl[(size_t)i * W + k] = Vl[(size_t)i * W + k];
  }
  // |U_j| (2-norm of the row, rounded up), then its maximum over all columns at or beyond each 128-column tile
  {
    double run = 0.0;
    for (int t = nf / 128 - 1; t >= 0; --t) {
      for (int j = 128 * t; j < 128 * (t + 1); ++j) {
        double s2 = 0.0;
        for (int i = 0; i < rp; ++i) s2 += u[(size_t)j * rp + i] * u[(size_t)j * rp + i];
        run = std::max(run, std::sqrt(s2) * (1.0 + 1e-12));
      }
      cu[t] = run;
    }
  }
  // staircase: columns of U a column tile's rows use at all (exact zeros beyond), in whole k chunks of the GEMM
  std::vector<int> kt(nf / 128, 0);
  double ksum = 0.0;
  for (int t = 0; t < nf / 128; ++t) {
    int last = 0;
    for (int j = 128 * t; j < 128 * (t + 1); ++j)
      for (int i = rp - 1; i >= last; --i)
        if (u[(size_t)j * rp + i] != 0.0) { last = i + 1; break; }
    kt[t] = ((last + G64_KC - 1) / G64_KC) * G64_KC;
    ksum += kt[t];
  }
  nnmpc_qp::Far f;
  f.W = W; f.r = r; f.rp = rp; f.U = f.Vx = f.Vl = f.cu = nullptr; f.kt = nullptr; f.ksum = ksum; f.efar = 0.0;
  // the factors are buffers of the handle's owner, given back at once when a set is refused or replaced
  DevRes& res = h->res;
  auto release = [&](nnmpc_qp::Far& g) {
    for (void* p : {(void*)g.U, (void*)g.Vx, (void*)g.Vl, (void*)g.cu, (void*)g.kt}) res.give_back(p);
    g.U = g.Vx = g.Vl = g.cu = nullptr; g.kt = nullptr;
  };
  auto hip = [](hipError_t e, const char* what) { if (e != hipSuccess) set_error("%s: %s", what, hipGetErrorString(e)); return e == hipSuccess ? NNMPC_OK : NNMPC_EHIP; };
#define FFCHK(x) do { if (int rc_ = (x)) { release(f); return rc_; } } while (0)
  FFCHK(res.upload(&f.U, u.data(), u.size()));
  FFCHK(res.upload(&f.Vx, vx.data(), vx.size()));
  FFCHK(res.upload(&f.Vl, vl.data(), vl.size()));
  FFCHK(res.upload(&f.cu, cu.data(), cu.size()));
  FFCHK(res.upload(&f.kt, kt.data(), kt.size()));
  // ---- verify on the device copies the passes will use: max |U [Vx | Vl] - [Kunc[W:] | -Pinv[W:, 0:W]]|
  {
    DevRes work;                                            // the result word (zeroed): freed on every way out of this block
    work.device = h->device;
    unsigned long long* em = nullptr;
    FFCHK(work.alloc(&em, 1));
    hipLaunchKernelGGL(far_verify_k, dim3(nf), dim3(256), rp * sizeof(double), h->stream, f.U, f.Vx, f.Vl, h->Kunc64, h->H64, W, rp, ka, np, em);
    unsigned long long bits = 0;
    FFCHK(hip(hipMemcpyAsync(&bits, em, 8, hipMemcpyDeviceToHost, h->stream), "hipMemcpyAsync"));
    FFCHK(hip(stream_sync(h->stream), "stream_sync"));
    double e;
    memcpy(&e, &bits, 8);
    f.efar = e;
    if (!(e < 1e-9)) { set_error("nnmpc_qp_set_farfield: max |U V' - M| = %.3e: the factors are not usable", e); release(f); return NNMPC_EINVAL; }
  }
#undef FFCHK
  h->far_missing.erase(std::remove(h->far_missing.begin(), h->far_missing.end(), W), h->far_missing.end());
  for (auto& g : h->far) if (g.W == W) { HIPCHK(stream_sync(h->stream)); release(g); g = f; return NNMPC_OK; }   // replaces the window's factors
  h->far.push_back(f);
  return NNMPC_OK;
  GUARD_END
}

int nnmpc_qp_farfield_missing(nnmpc_qp* h, int32_t* W) {
  if (!h || !W) { set_error("nnmpc_qp_farfield_missing: bad arguments"); return NNMPC_EINVAL; }
  *W = 0;
  if (!h->far_missing.empty()) { *W = h->far_missing.back(); h->far_missing.pop_back(); }   // handed out once: a window the caller cannot factor is not asked for again until met again
  return NNMPC_OK;
}

int nnmpc_qp_dims(nnmpc_qp* h, int32_t* n, int32_t* nu, int32_t* n_aug) {
  if (!h) { set_error("nnmpc_qp_dims: null handle"); return NNMPC_EINVAL; }
  if (n) *n = h->n;
  if (nu) *nu = h->nu;
  if (n_aug) *n_aug = h->n_aug;
  return NNMPC_OK;
}

int nnmpc_qp_set_profiling(nnmpc_qp* h, int32_t on) {
  if (!h) return NNMPC_EINVAL;
  h->profiling = on != 0;
  return NNMPC_OK;
}

int nnmpc_qp_get_stats(nnmpc_qp* h, nnmpc_qp_stats* out, int32_t reset) {
  if (!h || !out) return NNMPC_EINVAL;
  GUARD_BEGIN
  *out = h->stats;
  out->asm_e1max = h->asm_e1max; out->asm_e2max = h->asm_e2max;
  {
    std::vector<double> w(3 * (size_t)h->seg_max, 0.0);
    hipMemcpy(w.data(), h->asm_work, w.size() * sizeof(double), hipMemcpyDeviceToHost);
    double f = 0.0, b = 0.0, f32 = 0.0;
    for (size_t i = 0; i < w.size(); i += 3) { f += w[i]; b += w[i + 1]; f32 += w[i + 2]; }
    out->asm_lambda_flops = f; out->asm_lambda_bytes = b; out->asm_lambda32_flops = f32;
    if (reset) hipMemset(h->asm_work, 0, w.size() * sizeof(double));
  }
  {
    unsigned long long c = 0;
    hipMemcpy(&c, h->trsv_count, sizeof(c), hipMemcpyDeviceToHost);
    out->trsv_solves = (int64_t)c;
    if (reset) hipMemset(h->trsv_count, 0, sizeof(c));
  }
  if (reset) memset(&h->stats, 0, sizeof(h->stats));
  return NNMPC_OK;
  GUARD_END
}

int nnmpc_qp_solve_batch(nnmpc_qp* h, int32_t B, const double* x0, const double* lb, const double* ub,
                         double* u, uint32_t* active, int32_t* status, int32_t* iters, int32_t ptr_kind) {
  return nnmpc_qp_solve_batch_ex(h, B, x0, lb, ub, nullptr, u, active, status, iters, ptr_kind, NNMPC_OUT_SEQUENCE);
}

int nnmpc_qp_solve_batch_warm(nnmpc_qp* h, int32_t B, const double* x0, const double* lb, const double* ub,
                              const uint8_t* guess, double* u, uint32_t* active, int32_t* status,
                              int32_t* iters, int32_t ptr_kind) {
  return nnmpc_qp_solve_batch_ex(h, B, x0, lb, ub, guess, u, active, status, iters, ptr_kind, NNMPC_OUT_SEQUENCE);
}

// nnmpc_qp_solve_batch_ex, and with mult != nullptr nnmpc_qp_solve_batch_dual: the same segments, the same launches, then asm_mult_k on
// each segment's device-resident u and active words before anything is copied out.
static int solve_batch_impl(nnmpc_qp* h, int32_t B, const double* x0, const double* lb, const double* ub, const uint8_t* guess, double* u,
                            uint32_t* active, int32_t* status, int32_t* iters, int32_t ptr_kind, int32_t out_kind, double* mult) {
  if (!h || B < 0 || !x0 || !lb || !ub || !u) { set_error("nnmpc_qp_solve_batch: bad arguments"); return NNMPC_EINVAL; }
  if (out_kind != NNMPC_OUT_SEQUENCE && out_kind != NNMPC_OUT_FIRST_MOVE) { set_error("nnmpc_qp_solve_batch_ex: bad out_kind %d", out_kind); return NNMPC_EINVAL; }
  if (B == 0) return NNMPC_OK;
  GUARD_BEGIN
  HIPCHK(hipSetDevice(h->device));
  const int G = h->seg_max;
  const int ncol = out_kind == NNMPC_OUT_FIRST_MOVE ? h->nu : h->n;   // columns of the caller's u
  const size_t n = h->n, nu = h->nu, n_aug = h->n_aug, words = h->words;
  h->ldu = ncol; h->nout = ncol;
  CallScope call(h, EV_TOTAL);
  Staging stg{h->res, h->stream, ptr_kind == NNMPC_HOST};   // lax: any ptr_kind but NNMPC_HOST counts as NNMPC_DEVICE (callers may rely on it)
  for (int b0 = 0; b0 < B; b0 += G) {
    const int nb = std::min(G, B - b0);
    const double *x0d, *lbd, *ubd;
    const unsigned char* gd;
    double *ud, *md; uint32_t* ad; int32_t *sd, *idv;
    if (int rc = stg.in(&gd, guess, b0, nb, n, nnmpc_qp::SC_GUESS)) return rc;
    if (int rc = stg.in(&x0d, x0, b0, nb, n_aug, 0, h->in_stage)) return rc;
    if (int rc = stg.in(&lbd, lb, b0, nb, nu, 0, h->lb_d)) return rc;
    if (int rc = stg.in(&ubd, ub, b0, nb, nu, 0, h->ub_d)) return rc;
    if (int rc = stg.out(&ud, u, b0, nb, ncol, nnmpc_qp::SC_U)) return rc;
    // the multiplier kernel reads the segment's active words and status on the device, asked for or not
    if (int rc = stg.out(&ad, active, b0, nb, words, nnmpc_qp::SC_ACT, mult != nullptr)) return rc;
    if (int rc = stg.out(&sd, status, b0, nb, 1, nnmpc_qp::SC_ST, mult != nullptr)) return rc;
    if (int rc = stg.out(&idv, iters, b0, nb, 2, nnmpc_qp::SC_IT)) return rc;
    if (int rc = stg.out(&md, mult, b0, nb, n, nnmpc_qp::SC_MULT)) return rc;
    if (int rc = h->have_inverse && h->opts.method != 1 ? solve_segment_asm(h, nb, x0d, lbd, ubd, gd, ud, ad, sd, idv)
                                                        : solve_segment(h, nb, x0d, lbd, ubd, gd, ud, ad, sd, idv)) return rc;
    if (mult) if (int rc = launch_mult(h, nb, x0d, ud, ad, sd, md)) return rc;
    if (int rc = stg.copy_out()) return rc;
    if (stg.host) HIPCHK(stream_sync(h->stream));            // (the staging is the next segment's)
  }
  if (mult && !stg.host && stream_sync(h->stream) != hipSuccess) {   // the multipliers are there when the call returns
    set_error("nnmpc_qp_solve_batch_dual: the multiplier kernel failed");
    return NNMPC_EHIP;
  }
  return call.finish(NNMPC_OK);
  GUARD_END
}

int nnmpc_qp_solve_batch_ex(nnmpc_qp* h, int32_t B, const double* x0, const double* lb, const double* ub,
                            const uint8_t* guess, double* u, uint32_t* active, int32_t* status,
                            int32_t* iters, int32_t ptr_kind, int32_t out_kind) {
  return solve_batch_impl(h, B, x0, lb, ub, guess, u, active, status, iters, ptr_kind, out_kind, nullptr);
}

int nnmpc_qp_solve_batch_dual(nnmpc_qp* h, int32_t B, const double* x0, const double* lb, const double* ub,
                              const uint8_t* guess, double* u, uint32_t* active, int32_t* status,
                              int32_t* iters, double* mult, int32_t ptr_kind, int32_t out_kind) {
  if (mult && out_kind == NNMPC_OUT_FIRST_MOVE) {
    set_error("nnmpc_qp_solve_batch_dual: multipliers need the whole sequence, which NNMPC_OUT_FIRST_MOVE does not form in the caller's u");
    return NNMPC_EINVAL;
  }
  return solve_batch_impl(h, B, x0, lb, ub, guess, u, active, status, iters, ptr_kind, out_kind, mult);
}

int nnmpc_qp_multipliers(nnmpc_qp* h, int32_t B, const double* x0, const double* u, const uint32_t* active,
                         const int32_t* status, double* mult, int32_t ptr_kind) {
  if (!h || B < 0 || !x0 || !u || !active || !mult || (ptr_kind != NNMPC_HOST && ptr_kind != NNMPC_DEVICE)) {
    set_error("nnmpc_qp_multipliers: bad arguments");
    return NNMPC_EINVAL;
  }
  if (B == 0) return NNMPC_OK;
  GUARD_BEGIN
  HIPCHK(hipSetDevice(h->device));
  CallScope call(h);
  Staging stg{h->res, h->stream, ptr_kind == NNMPC_HOST};
  const int G = stg.host ? std::min(h->seg_max, (int)B) : B;   // device pointers: one launch over the batch
  for (int b0 = 0; b0 < B; b0 += G) {
    const int nb = std::min(G, B - b0);
    const double *x0d, *ud; const uint32_t* ad; const int32_t* sd; double* md;
    if (int rc = stg.in(&x0d, x0, b0, nb, h->n_aug, nnmpc_qp::SC_X0)) return rc;
    if (int rc = stg.in(&ud, u, b0, nb, h->n, nnmpc_qp::SC_U)) return rc;
    if (int rc = stg.in(&ad, active, b0, nb, h->words, nnmpc_qp::SC_ACT)) return rc;
    if (int rc = stg.in(&sd, status, b0, nb, 1, nnmpc_qp::SC_ST)) return rc;
    if (int rc = stg.out(&md, mult, b0, nb, h->n, nnmpc_qp::SC_MULT)) return rc;
    if (int rc = launch_mult(h, nb, x0d, ud, ad, sd, md)) return rc;
    if (int rc = stg.copy_out()) return rc;
    HIPCHK(stream_sync(h->stream));
  }
  return call.finish(NNMPC_OK);
  GUARD_END
}

// The problems of a segment sorted into the two instances of sens_k / adj_k from one read-back of the counts: list (device) holds
// the nl problems of the LDS instance (sets of at most SENS_M_LDS bounds, and those beyond SENS_M_MAX, which it flags), then the ns
// of the slab instance; hi = the largest active variable of any problem that is computed (-1: none).
struct SensSort { int* cnt; int* list; std::vector<int> hcnt, hlist; int nl, ns, hi; };
static int sens_sort(nnmpc_qp* h, SensSort& w, int nb, const uint32_t* act) {
  hipLaunchKernelGGL(sens_count_k, dim3((nb + 3) / 4), dim3(256), 0, h->stream, act, h->words, h->n, h->nu, nb, w.cnt);
  HIPCHK(hipGetLastError());
  w.hcnt.resize(2 * (size_t)nb); w.hlist.resize(nb);
  HIPCHK(hipMemcpyAsync(w.hcnt.data(), w.cnt, 2 * (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(stream_sync(h->stream));
  int nl = 0, ns = 0, hi = -1;
  for (int b = 0; b < nb; ++b) {
    const int m = w.hcnt[2 * b];
    if (m > SENS_M_LDS && m <= SENS_M_MAX) ++ns;
    if (m <= SENS_M_MAX) hi = std::max(hi, w.hcnt[2 * b + 1]);
  }
  nl = nb - ns;
  for (int b = 0, il = 0, is = nl; b < nb; ++b) {
    const int m = w.hcnt[2 * b];
    if (m > SENS_M_LDS && m <= SENS_M_MAX) w.hlist[is++] = b; else w.hlist[il++] = b;
  }
  HIPCHK(hipMemcpyAsync(w.list, w.hlist.data(), (size_t)nb * sizeof(int), hipMemcpyHostToDevice, h->stream));
  w.nl = nl; w.ns = ns; w.hi = hi;
  return NNMPC_OK;
}

// One segment of nnmpc_qp_sensitivity on device pointers: nb problems, D directions each (qp_sens.h).  du: nb D x n (seq) or x nu.
struct SensWork {
  bool seq; int D;
  SensSort s; double* xp; double* T; double* lam; double* X; uint32_t* arep;
};
static int sens_segment(nnmpc_qp* h, SensWork& w, int nb, const uint32_t* act, const int32_t* st, const double* dx0, const double* dlb,
                        const double* dub, double* du, double* dmult, int32_t* flag) {
  const int n = h->n, np = h->np, nu = h->nu, n_aug = h->n_aug, ka = h->ka, D = w.D;
  const size_t rows = (size_t)nb * D, mpad = (rows + 127) / 128 * 128;
  // the host sorts the segment into the two instances from one read-back of the counts (and takes the window of the second product)
  if (int rc = sens_sort(h, w.s, nb, act)) return rc;
  const int nl = w.s.nl, ns = w.s.ns, hi = w.s.hi;
  const int W = std::min(np, (hi + 16) / 16 * 16);           // columns of LAM in use (0: no active bound in the segment)
  if (w.seq) {
    hipLaunchKernelGGL(sens_pad_k, dim3((unsigned)std::min<size_t>((mpad * ka + 255) / 256, 65535)), dim3(256), 0, h->stream,
                       w.xp, dx0, rows, n_aug, ka, mpad);
    HIPCHK(hipGetLastError());
    gemm64(h, w.T, np, w.xp, ka, h->Kunc64, ka, (int)mpad, np, ka);                      // T = dX0 Kunc'
    if (W > 0) HIPCHK(hipMemset2DAsync(w.lam, (size_t)np * 8, 0, (size_t)W * 8, mpad, h->stream));
  }
  SensArgs a;
  a.H64 = h->H64; a.Kunc64 = h->Kunc64; a.active = act; a.status = st; a.dx0 = dx0; a.dlb = dlb; a.dub = dub;
  a.slab = nullptr; a.lam = w.seq ? w.lam : nullptr; a.ldl = np; a.du0 = w.seq ? nullptr : du; a.flag = flag;
  a.n = n; a.np = np; a.nu = nu; a.n_aug = n_aug; a.ka = ka; a.words = h->words; a.D = D;
  if (nl > 0) {
    a.list = w.s.list; a.count = nl;
    EvScope es(h, EV_SENS, 0.0);
    hipLaunchKernelGGL(sens_k<false>, dim3(nl), dim3(SENS_THREADS), sens_lds_bytes<false>(), h->stream, a);
    HIPCHK(hipGetLastError());
  }
  if (ns > 0) {
    const int pool = std::min(ns, 64);                       // workgroups, each with a slab of 2.4 MB, that walk the list together
    if (int rc = h->res.slot(nnmpc_qp::SC_S_SLAB, &a.slab, (size_t)pool * SENS_SLAB * 8)) return rc;
    a.list = w.s.list + nl; a.count = ns;
    EvScope es(h, EV_SENS, 0.0);
    hipLaunchKernelGGL(sens_k<true>, dim3(pool), dim3(SENS_THREADS), sens_lds_bytes<true>(), h->stream, a);
    HIPCHK(hipGetLastError());
  }
  h->stats.sens_lds_problems += nl; h->stats.sens_slab_problems += ns;
  if (w.seq) {
    if (W > 0) gemm64(h, w.X, np, w.lam, np, h->H64, np, (int)mpad, np, W);             // X = LAM Hinv[:, 0:W]'
    hipLaunchKernelGGL(sens_epilogue_k, dim3((unsigned)rows), dim3(256), 0, h->stream, du, w.T, W > 0 ? w.X : nullptr, (size_t)np, act,
                       flag, dlb, dub, dmult ? w.arep : nullptr, n, nu, h->words, D);
    HIPCHK(hipGetLastError());
    if (dmult)
      if (int rc = launch_mult(h, (int)rows, dx0, du, w.arep, nullptr, dmult)) return rc;
  }
  return NNMPC_OK;
}

int nnmpc_qp_sensitivity(nnmpc_qp* h, int32_t B, int32_t D, const uint32_t* active, const int32_t* status, const double* dx0,
                         const double* dlb, const double* dub, double* du, double* dmult, int32_t* flag,
                         int32_t ptr_kind, int32_t out_kind) {
  if (!h || B < 0 || D < 1 || !active || !dx0 || !du || (ptr_kind != NNMPC_HOST && ptr_kind != NNMPC_DEVICE) ||
      (out_kind != NNMPC_OUT_SEQUENCE && out_kind != NNMPC_OUT_FIRST_MOVE)) {
    set_error("nnmpc_qp_sensitivity: bad arguments");
    return NNMPC_EINVAL;
  }
  if (dmult && out_kind == NNMPC_OUT_FIRST_MOVE) {
    set_error("nnmpc_qp_sensitivity: dmult needs the whole sequence, which NNMPC_OUT_FIRST_MOVE does not form");
    return NNMPC_EINVAL;
  }
  if (!h->have_inverse) {
    set_error("nnmpc_qp_sensitivity: needs an accepted inverse (nnmpc_qp_set_inverse)");
    return NNMPC_EINVAL;
  }
  if (B == 0) return NNMPC_OK;
  GUARD_BEGIN
  HIPCHK(hipSetDevice(h->device));
  const int n = h->n, np = h->np, nu = h->nu, n_aug = h->n_aug, ka = h->ka, words = h->words;
  const bool seq = out_kind == NNMPC_OUT_SEQUENCE;
  const int ncol = seq ? n : nu;
  // rows (problem, direction) of a segment: the three np-wide row buffers of the sequence output stay within 1 GiB
  const long long rowcap = seq ? std::max<long long>(128, (1ll << 30) / (3ll * np * 8)) : std::max<long long>(h->seg_max, 1024);
  const int G = (int)std::min<long long>(std::min<long long>(B, h->seg_max), std::max<long long>(1, rowcap / D));
  if ((long long)G * D > 0x7fffff00ll) { set_error("nnmpc_qp_sensitivity: D = %d is too large", D); return NNMPC_EINVAL; }
  const size_t rmax = (size_t)G * D, mpad = (rmax + 127) / 128 * 128;
  DevRes& res = h->res;
  SensWork w;
  w.seq = seq; w.D = D; w.s.cnt = nullptr; w.s.list = nullptr; w.xp = w.T = w.lam = w.X = nullptr; w.arep = nullptr;
  if (int rc = res.slot(nnmpc_qp::SC_S_CNT, &w.s.cnt, 2 * (size_t)G * 4)) return rc;
  if (int rc = res.slot(nnmpc_qp::SC_S_LIST, &w.s.list, (size_t)G * 4)) return rc;
  if (seq) {
    if (int rc = res.slot(nnmpc_qp::SC_S_XP, &w.xp, mpad * ka * 8)) return rc;
    if (int rc = res.slot(nnmpc_qp::SC_S_T, &w.T, mpad * np * 8)) return rc;
    if (int rc = res.slot(nnmpc_qp::SC_S_LAM, &w.lam, mpad * np * 8)) return rc;
    if (int rc = res.slot(nnmpc_qp::SC_S_X, &w.X, mpad * np * 8)) return rc;
    if (dmult) if (int rc = res.slot(nnmpc_qp::SC_S_AREP, &w.arep, rmax * words * 4)) return rc;
  }
  CallScope call(h, EV_SENS_TOTAL);
  Staging stg{res, h->stream, ptr_kind == NNMPC_HOST};
  for (int b0 = 0; b0 < B; b0 += G) {
    const int nb = std::min(G, B - b0);
    const size_t r0 = (size_t)b0 * D, nr = (size_t)nb * D;
    const uint32_t* ad; const int32_t* sd; const double *xd, *lbd, *ubd;
    double *dud, *dmd; int32_t* fd;
    if (int rc = stg.in(&ad, active, b0, nb, words, nnmpc_qp::SC_ACT)) return rc;
    if (int rc = stg.in(&sd, status, b0, nb, 1, nnmpc_qp::SC_ST)) return rc;
    if (int rc = stg.in(&xd, dx0, r0, nr, n_aug, nnmpc_qp::SC_X0)) return rc;
    if (int rc = stg.in(&lbd, dlb, r0, nr, nu, nnmpc_qp::SC_LB)) return rc;
    if (int rc = stg.in(&ubd, dub, r0, nr, nu, nnmpc_qp::SC_UB)) return rc;
    if (int rc = stg.out(&dud, du, r0, nr, ncol, nnmpc_qp::SC_U)) return rc;
    if (int rc = stg.out(&dmd, dmult, r0, nr, n, nnmpc_qp::SC_MULT)) return rc;
    if (int rc = stg.out(&fd, flag, b0, nb, 1, nnmpc_qp::SC_FLAG, true)) return rc;   // the kernels write it, asked for or not
    if (int rc = sens_segment(h, w, nb, ad, sd, xd, lbd, ubd, dud, dmd, fd)) return rc;
    if (int rc = stg.copy_out()) return rc;
    HIPCHK(stream_sync(h->stream));                          // (the staging and the row buffers are the next segment's)
  }
  return call.finish(NNMPC_OK);
  GUARD_END
}

// One segment of nnmpc_qp_adjoint on device pointers: nb problems, D cotangents each (qp_adj.h).  v: nb D x n (seq) or x nu.
struct AdjWork {
  bool seq; int D, kap;
  SensSort s; double* Vp; double* Y; double* GX; const double* KT;
};
static int adj_segment(nnmpc_qp* h, AdjWork& w, int nb, const uint32_t* act, const int32_t* st, const double* v, double* gx0, double* glb,
                       double* gub, double* gbound, int32_t* flag) {
  const int n = h->n, np = h->np, nu = h->nu, n_aug = h->n_aug, ka = h->ka, D = w.D;
  const size_t rows = (size_t)nb * D, mpad = (rows + 127) / 128 * 128;
  if (int rc = sens_sort(h, w.s, nb, act)) return rc;
  const int nl = w.s.nl, ns = w.s.ns;
  const int W = std::min(np, (w.s.hi + 64) / 64 * 64);       // columns of Y in use (0: no active bound in the segment)
  if (w.seq) {
    hipLaunchKernelGGL(sens_pad_k, dim3((unsigned)std::min<size_t>((mpad * np + 255) / 256, 65535)), dim3(256), 0, h->stream,
                       w.Vp, v, rows, n, np, mpad);
    HIPCHK(hipGetLastError());
    if (W > 0) gemm64(h, w.Y, np, w.Vp, np, h->H64, np, (int)mpad, W, np);               // Y = V Hinv[0:W, :]'
  }
  AdjArgs a;
  a.H64 = h->H64; a.Kunc64 = h->Kunc64; a.active = act; a.status = st; a.v = v; a.slab = nullptr;
  a.vp = w.seq ? w.Vp : nullptr; a.y = w.seq ? w.Y : nullptr; a.ld = np; a.gx0 = w.seq ? nullptr : gx0;
  a.glb = glb; a.gub = gub; a.gbound = gbound; a.flag = flag;
  a.n = n; a.np = np; a.nu = nu; a.n_aug = n_aug; a.ka = ka; a.words = h->words; a.D = D;
  if (nl > 0) {
    a.list = w.s.list; a.count = nl;
    EvScope es(h, EV_ADJ, 0.0);
    hipLaunchKernelGGL(adj_k<false>, dim3(nl), dim3(SENS_THREADS), sens_lds_bytes<false>(), h->stream, a);
    HIPCHK(hipGetLastError());
  }
  if (ns > 0) {
    const int pool = std::min(ns, 64);                       // as sens_segment's
    if (int rc = h->res.slot(nnmpc_qp::SC_S_SLAB, &a.slab, (size_t)pool * SENS_SLAB * 8)) return rc;
    a.list = w.s.list + nl; a.count = ns;
    EvScope es(h, EV_ADJ, 0.0);
    hipLaunchKernelGGL(adj_k<true>, dim3(pool), dim3(SENS_THREADS), sens_lds_bytes<true>(), h->stream, a);
    HIPCHK(hipGetLastError());
  }
  h->stats.adj_lds_problems += nl; h->stats.adj_slab_problems += ns;
  if (w.seq) {
    gemm64(h, w.GX, w.kap, w.Vp, np, w.KT, np, (int)mpad, w.kap, np);                    // GX = Z KuncT'
    hipLaunchKernelGGL(adj_epilogue_k, dim3((unsigned)rows), dim3(256), 0, h->stream, gx0, w.GX, (size_t)w.kap, flag, n_aug, D);
    HIPCHK(hipGetLastError());
  }
  return NNMPC_OK;
}

int nnmpc_qp_adjoint(nnmpc_qp* h, int32_t B, int32_t D, const uint32_t* active, const int32_t* status, const double* v,
                     double* gx0, double* glb, double* gub, double* gbound, int32_t* flag, int32_t ptr_kind, int32_t in_kind) {
  if (!h || B < 0 || D < 1 || !active || !v || !gx0 || (ptr_kind != NNMPC_HOST && ptr_kind != NNMPC_DEVICE) ||
      (in_kind != NNMPC_OUT_SEQUENCE && in_kind != NNMPC_OUT_FIRST_MOVE)) {
    set_error("nnmpc_qp_adjoint: bad arguments");
    return NNMPC_EINVAL;
  }
  if (!h->have_inverse) {
    set_error("nnmpc_qp_adjoint: needs an accepted inverse (nnmpc_qp_set_inverse)");
    return NNMPC_EINVAL;
  }
  if (B == 0) return NNMPC_OK;
  GUARD_BEGIN
  HIPCHK(hipSetDevice(h->device));
  const int n = h->n, np = h->np, nu = h->nu, n_aug = h->n_aug, ka = h->ka, words = h->words;
  const bool seq = in_kind == NNMPC_OUT_SEQUENCE;
  const int ncol = seq ? n : nu, kap = (n_aug + 63) / 64 * 64;
  // rows (problem, cotangent) of a segment: the row buffers of the sequence input (V / Z, Y, GX) stay within 1 GiB
  const long long rowcap = seq ? std::max<long long>(128, (1ll << 30) / ((2ll * np + kap) * 8)) : std::max<long long>(h->seg_max, 1024);
  const int G = (int)std::min<long long>(std::min<long long>(B, h->seg_max), std::max<long long>(1, rowcap / D));
  if ((long long)G * D > 0x7fffff00ll) { set_error("nnmpc_qp_adjoint: D = %d is too large", D); return NNMPC_EINVAL; }
  const size_t rmax = (size_t)G * D, mpad = (rmax + 127) / 128 * 128;
  DevRes& res = h->res;
  AdjWork w;
  w.seq = seq; w.D = D; w.kap = kap; w.s.cnt = nullptr; w.s.list = nullptr; w.Vp = w.Y = w.GX = nullptr; w.KT = nullptr;
  if (int rc = res.slot(nnmpc_qp::SC_S_CNT, &w.s.cnt, 2 * (size_t)G * 4)) return rc;
  if (int rc = res.slot(nnmpc_qp::SC_S_LIST, &w.s.list, (size_t)G * 4)) return rc;
  if (seq) {
    if (int rc = res.slot(nnmpc_qp::SC_S_T, &w.Vp, mpad * np * 8)) return rc;
    if (int rc = res.slot(nnmpc_qp::SC_S_LAM, &w.Y, mpad * np * 8)) return rc;
    if (int rc = res.slot(nnmpc_qp::SC_S_X, &w.GX, mpad * kap * 8)) return rc;
    double* kt = nullptr;
    if (int rc = res.slot(nnmpc_qp::SC_A_KT, &kt, (size_t)kap * np * 8)) return rc;
    if (!h->kunct_ok) {
      hipLaunchKernelGGL(adj_transpose_k, dim3((unsigned)std::min<size_t>(((size_t)kap * np + 255) / 256, 65535)), dim3(256), 0, h->stream,
                         kt, h->Kunc64, np, ka, n_aug, kap);
      HIPCHK(hipGetLastError());
      h->kunct_ok = true;
    }
    w.KT = kt;
  }
  CallScope call(h, EV_ADJ_TOTAL);
  Staging stg{res, h->stream, ptr_kind == NNMPC_HOST};
  for (int b0 = 0; b0 < B; b0 += G) {
    const int nb = std::min(G, B - b0);
    const size_t r0 = (size_t)b0 * D, nr = (size_t)nb * D;
    const uint32_t* ad; const int32_t* sd; const double* vd;
    double *gxd, *gld, *gud, *gbd; int32_t* fd;
    if (int rc = stg.in(&ad, active, b0, nb, words, nnmpc_qp::SC_ACT)) return rc;
    if (int rc = stg.in(&sd, status, b0, nb, 1, nnmpc_qp::SC_ST)) return rc;
    if (int rc = stg.in(&vd, v, r0, nr, ncol, nnmpc_qp::SC_X0)) return rc;
    if (int rc = stg.out(&gxd, gx0, r0, nr, n_aug, nnmpc_qp::SC_U)) return rc;
    if (int rc = stg.out(&gld, glb, r0, nr, nu, nnmpc_qp::SC_LB)) return rc;
    if (int rc = stg.out(&gud, gub, r0, nr, nu, nnmpc_qp::SC_UB)) return rc;
    if (int rc = stg.out(&gbd, gbound, r0, nr, n, nnmpc_qp::SC_MULT)) return rc;
    if (int rc = stg.out(&fd, flag, b0, nb, 1, nnmpc_qp::SC_FLAG, true)) return rc;   // the kernels write it, asked for or not
    if (int rc = adj_segment(h, w, nb, ad, sd, vd, gxd, gld, gud, gbd, fd)) return rc;
    if (int rc = stg.copy_out()) return rc;
    HIPCHK(stream_sync(h->stream));                          // (the staging and the row buffers are the next segment's)
  }
  return call.finish(NNMPC_OK);
  GUARD_END
}

int nnmpc_qp_debug_factor_solve(nnmpc_qp* h, int32_t B, const float* dvec, const float* mask,
                                const float* rhs, float* sol) {
  if (!h || B <= 0 || B > h->slots || !dvec || !mask || !rhs || !sol) { set_error("debug_factor_solve: bad arguments"); return NNMPC_EINVAL; }
  GUARD_BEGIN
  HIPCHK(hipSetDevice(h->device));
  CallScope call(h);
  QpDev& d = h->d;
  const int rows = h->slots;
  std::vector<float> dv((size_t)rows * h->np, 0.f), mk((size_t)rows * h->np, 1.f), rh((size_t)rows * h->np, 0.f);
  std::vector<int> fl(rows, 0);
  for (int p = 0; p < B; ++p) {
    fl[p] = 1;
    for (int r = 0; r < h->n; ++r) {
      dv[(size_t)p * h->np + r] = dvec[(size_t)p * h->n + r];
      mk[(size_t)p * h->np + r] = mask[(size_t)p * h->n + r];
      rh[(size_t)p * h->np + r] = rhs[(size_t)p * h->n + r];
    }
  }
  HIPCHK(hipMemcpy(d.dvec, dv.data(), dv.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d.mask, mk.data(), mk.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d.rhs, rh.data(), rh.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d.f_factor, fl.data(), rows * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(d.fail, 0, rows * 4));
  factor_dispatch(h, rows, B);
  solve_dispatch(h, rows, d.f_factor);
  HIPCHK(stream_sync(h->stream));
  HIPCHK(hipGetLastError());
  std::vector<float> so((size_t)rows * h->np);
  HIPCHK(hipMemcpy(so.data(), d.sol, so.size() * 4, hipMemcpyDeviceToHost));
  for (int p = 0; p < B; ++p)
    for (int r = 0; r < h->n; ++r) sol[(size_t)p * h->n + r] = so[(size_t)p * h->np + r];
  return call.finish(NNMPC_OK);
  GUARD_END
}

int nnmpc_qp_debug_factor_fail(nnmpc_qp* h, int32_t B, int32_t* fail) {
  if (!h || B <= 0 || B > h->slots || !fail) { set_error("debug_factor_fail: bad arguments"); return NNMPC_EINVAL; }
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(stream_sync(h->stream));
  HIPCHK(hipMemcpy(fail, h->d.fail, (size_t)B * 4, hipMemcpyDeviceToHost));
  return NNMPC_OK;
}

int nnmpc_qp_debug_predict(nnmpc_qp* h, int32_t B, const double* x0, const double* lb, const double* ub, int32_t iters, int32_t wide,
                           uint8_t* state, int32_t* info, double* L) {
  if (!h || B <= 0 || B > h->seg_max || !x0 || !lb || !ub || !state || !info || !L || iters < 0 || iters > PRED_MAXIT || wide < -1 || wide > 1) {
    set_error("debug_predict: bad arguments"); return NNMPC_EINVAL;
  }
  if (!h->have_inverse) { set_error("debug_predict: needs nnmpc_qp_set_inverse first"); return NNMPC_EINVAL; }
  if (!(h->pred[0].L > 0.0)) { set_error("debug_predict: the handle has no predictor window (n = %d, nu = %d)", h->n, h->nu); return NNMPC_EINVAL; }
  if (wide == 1 && !(h->pred[1].L > 0.0)) { set_error("debug_predict: the handle has no 1024-column window (n = %d, nu = %d)", h->n, h->nu); return NNMPC_EINVAL; }
  GUARD_BEGIN
  HIPCHK(hipSetDevice(h->device));
  CallScope call(h);
  hipStream_t s = h->stream;
  const int nprob = B, segp = ((nprob + 127) / 128) * 128;
  HIPCHK(hipMemcpyAsync(h->in_stage, x0, (size_t)nprob * h->n_aug * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(h->lb_d, lb, (size_t)nprob * h->nu * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(h->ub_d, ub, (size_t)nprob * h->nu * 8, hipMemcpyHostToDevice, s));
  // what solve_segment_asm does up to the predictor's launch: x0 padded, x_unc for the window's columns, the bound states cleared
  hipLaunchKernelGGL(pad_x0_k, dim3(512), dim3(256), 0, s, h->x0_64, h->x0_32, h->in_stage, nprob, h->n_aug, h->ka, segp);
  int Wx = PRED_W;
  gemm64(h, h->asm_xunc, h->np, h->x0_64, h->ka, h->Kunc64, h->ka, segp, Wx, h->ka);
  AsmDev a;
  memset(&a, 0, sizeof(a));
  a.n = h->n; a.np = h->np; a.nu = h->nu; a.nseg = nprob; a.Wx = Wx;
  a.lb = h->lb_d; a.ub = h->ub_d; a.xunc = h->asm_xunc; a.st = h->asm_st;
  HIPCHK(hipMemsetAsync(h->asm_st, 0, (size_t)nprob * h->n, s));
  int count = -1;
  if (wide < 0) {
    wide = 0;
    if (h->pred[1].L > 0.0) {
      const int rc = predictor_extent(h, a, nprob, &count);
      if (rc) return rc;
      wide = count * 4 > nprob;
    }
  }
  if (wide) {
    gemm64(h, h->asm_xunc + Wx, h->np, h->x0_64, h->ka, h->Kunc64 + (size_t)Wx * h->ka, h->ka, segp, PRED_W2 - Wx, h->ka);
    Wx = PRED_W2; a.Wx = Wx;
  }
  int W = 0, MR = 0;
  double flops_per_it = 0.0;
  const int rc = launch_predictor(h, a, nprob, iters, wide, &W, &MR, &flops_per_it);
  if (rc) return rc;
  HIPCHK(stream_sync(s));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(state, h->asm_st, (size_t)nprob * h->n, hipMemcpyDeviceToHost));
  info[0] = W; info[1] = MR; info[2] = count; info[3] = wide;
  *L = h->pred[wide].L;
  return call.finish(NNMPC_OK);
  GUARD_END
}

int nnmpc_qp_debug_gemm(nnmpc_qp* h, int32_t kind, int32_t M, int32_t N, int32_t K, const void* A, int64_t lda, int64_t a_rows,
                        const void* B, int64_t ldb, void* C, int64_t ldc, int64_t c_rows, const int32_t* rowphase, int32_t want,
                        const int32_t* kdyn, int32_t kblocks, const int32_t* mdyn, const int32_t* rowmap, int32_t* info) {
#define GEMM_BAD(...) do { set_error("nnmpc_qp_debug_gemm: " __VA_ARGS__); return NNMPC_EINVAL; } while (0)
  if (!h || !A || !B || !C || !info) GEMM_BAD("null handle, operand or info");
  if (kind < 0 || kind > 4) GEMM_BAD("kind %d (0 .. 4)", kind);
  const bool f32 = kind >= 3;
  const int T = (kind == 1 || kind == 3) ? 128 : 64, kc = f32 ? KC : G64_KC, el = f32 ? 4 : 8;
  if (M < 1 || N < 1 || K < kc || M > (1 << 20) || N > (1 << 16) || K > (1 << 16)) GEMM_BAD("M = %d, N = %d, K = %d out of range", M, N, K);
  // what each kernel needs of the shape (kind 0: what either kernel of gemm64 can run without leaving its operands -- the 64 x 64
  // kernel walks K in whole chunks of 16 and drops a remainder; gemm64's callers pad K)
  if (kind == 0 ? (M % 64 || N % 64) : f32 ? (N % T || K % kc) : (M % T || N % T || K % kc))
    GEMM_BAD("M = %d, N = %d, K = %d off the grid of kind %d (tiles of %d, K in chunks of %d)", M, N, K, kind, T, kc);
  if (f32 && !kdyn) GEMM_BAD("kind %d needs kdyn", kind);
  if (f32 && (rowphase || mdyn || rowmap)) GEMM_BAD("kind %d has no rowphase, mdyn or rowmap", kind);
  if (kind == 2 && rowmap) GEMM_BAD("kind 2 (the 64 x 64 kernel) has no rowmap");
  if (lda < K || ldb < K || ldc < N) GEMM_BAD("a leading dimension shorter than its row (lda = %lld, ldb = %lld, ldc = %lld; K = %d, N = %d)",
                                              (long long)lda, (long long)ldb, (long long)ldc, K, N);
  const int vec = 16 / el;                                  // the kernels load 16 bytes at a time
  if (lda % vec || ldb % vec) GEMM_BAD("lda = %lld, ldb = %lld: rows of A and B must start on 16 bytes", (long long)lda, (long long)ldb);
  const int64_t mr = ((int64_t)M + T - 1) / T * T;          // rows the grid covers
  if (a_rows < (rowmap ? 1 : mr) || c_rows < (rowmap ? 1 : mr)) GEMM_BAD("A (%lld rows) or C (%lld rows) shorter than the %lld rows of the grid",
                                                                         (long long)a_rows, (long long)c_rows, (long long)mr);
  if (rowmap)
    for (int i = 0; i < M; ++i)
      if (rowmap[i] >= a_rows || rowmap[i] >= c_rows) GEMM_BAD("rowmap[%d] = %d beyond the arrays (%lld, %lld rows)", i, rowmap[i], (long long)a_rows, (long long)c_rows);
  if (mdyn && (*mdyn < 0 || *mdyn > M)) GEMM_BAD("*mdyn = %d outside 0 .. M", *mdyn);
  const size_t na = (size_t)(a_rows - 1) * lda + K, nb = (size_t)(N - 1) * ldb + K, nc = (size_t)(c_rows - 1) * ldc + N;   // elements in use
  if (na * el >= ((size_t)1 << 32) || nb * el >= ((size_t)1 << 32) || nc * el >= ((size_t)1 << 32)) GEMM_BAD("an operand of 4 GB or more");
  GUARD_BEGIN
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  HIPCHK(stream_sync(s));
  DevRes scratch;                                            // the call's own device memory: freed on every way out
  scratch.device = h->device;
  char *dA = nullptr, *dB = nullptr, *dC = nullptr;
  int *dphase = nullptr, *dk = nullptr, *dm = nullptr, *dmap = nullptr;
  const size_t nk = kdyn ? ((kblocks || f32) ? (size_t)(mr / 64) : 1) : 0;
  int rc = scratch.upload(&dA, (const char*)A, na * el);
  if (!rc) rc = scratch.upload(&dB, (const char*)B, nb * el);
  if (!rc) rc = scratch.upload(&dC, (const char*)C, nc * el);
  if (!rc && rowphase) rc = scratch.upload(&dphase, rowphase, (size_t)M);
  if (!rc && kdyn) rc = scratch.upload(&dk, kdyn, nk);
  if (!rc && mdyn) rc = scratch.upload(&dm, mdyn, (size_t)1);
  if (!rc && rowmap) rc = scratch.upload(&dmap, rowmap, (size_t)M);
  if (rc) return rc;
  int which = 0, nwg = 0, kper = 0;
  if (f32) {
    float* c32 = (float*)dC; const float *a32 = (const float*)dA, *b32 = (const float*)dB;
    if (kind == 3) launch_xh32_nb<128>(s, c32, (size_t)ldc, a32, (size_t)lda, b32, (size_t)ldb, M, N, K, dk);
    else launch_xh32_nb<64>(s, c32, (size_t)ldc, a32, (size_t)lda, b32, (size_t)ldb, M, N, K, dk);
    which = kind; nwg = (N / T) * (int)(mr / T); kper = T / 64;
  } else {
    double* c64 = (double*)dC; const double *a64 = (const double*)dA, *b64 = (const double*)dB;
    if (kind == 0) {
      // the solves' own entry, flag and all.  A refusal must not outlive this call: the handle's flag is left as it was found
      // (a solve reads and clears it at its own check).
      const bool had = h->gemm_error;
      which = gemm64(h, c64, (size_t)ldc, a64, (size_t)lda, b64, (size_t)ldb, M, N, K, dphase, want, dk, dm, kblocks != 0, dmap, &nwg);
      h->gemm_error = had;
      if (which == GEMM64_REFUSED) { info[0] = 0; info[1] = 0; info[2] = 0; info[3] = 0; return NNMPC_EINVAL; }   // (gemm64's message)
    } else if (kind == 1) {
      which = GEMM64_T128;
      nwg = launch_gemm64_t128(s, c64, (size_t)ldc, a64, (size_t)lda, b64, (size_t)ldb, M, N, K, dphase, want, dk, dm, kblocks != 0, dmap);
    } else {
      which = GEMM64_K64;
      nwg = launch_gemm64_k64(s, c64, (size_t)ldc, a64, (size_t)lda, b64, (size_t)ldb, M, N, K, dphase, want, dk, dm, kblocks != 0);
    }
    kper = (kdyn && kblocks) ? (which == GEMM64_T128 ? 2 : 1) : 0;
  }
  HIPCHK(stream_sync(s));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(C, dC, nc * el, hipMemcpyDeviceToHost));
  info[0] = which; info[1] = nwg; info[2] = kper; info[3] = (which == 1 || which == 3) ? 128 : 64;
  return NNMPC_OK;
  GUARD_END
#undef GEMM_BAD
}

}  // extern "C"
