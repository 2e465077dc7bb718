// Lock-step closed-loop evaluation (gfx950): online_simulation (lib/linearMPC.py:703-718) for every (controller, scenario,
// noise seed) instance of an evaluation at once -- see include/nnmpc.h (nnmpc_cl_*).  Per step:
//   cl_filter_k    filter update and the target problem's reduction (one workgroup per instance)
//   ts_solve_k     the reduced target QPs of all instances (nnmpc_ts_launch_internal, one wave per instance)
//   cl_expand_k    xs, the regulator's inputs (MPC), Kaug z + us (SATDLQR), us (US), the two NN input rows (NN) or the one (NN_UNSTD)
//   cl_nn_layer_k  grouped NN forward: ONE launch per layer index for all networks, structured and unstructured (workgroup = network x 64 columns)
//   nnmpc_qp_solve_batch_ex per MPC slot on the borrowed handle's stream (first moves, warm-started), beside the NN layers
//   cl_post_k      u (NN combine + clip, NN_UNSTD clip, SATDLQR clip, MPC first move + us), stage cost, running mean, plant step, records
// Shared matrices are read by all instances from L2; a thread owns one output element and walks a stored transpose so that
// the lanes of a wave read consecutive doubles.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "dev_res.h"

using namespace nnmpc;

namespace {

constexpr int CL_THREADS = 256;
constexpr int NN_RB = 8;          // rows of a network per pass of cl_nn_layer_k (register accumulators per thread)
constexpr int NN_KS = 4;          // K slices of a workgroup (4 waves x 64 columns), summed in a fixed order
constexpr int NN_MAXK = 2048;     // LDS: NN_RB x K floats
constexpr int CL_EV_BLOCK = 256;  // steps whose phase events are alive at once (nnmpc_cl_run)

struct SlotDev {                  // per slot, device copy
  int kind, base, count, n, words, with_uprev, row0;
  const double* Kt;               // SATDLQR: Kaug' ((nx + nu) x nu)
  const double* xscale;           // NN: nx
  const double* first;            // MPC: first moves [count][nu]
  const uint32_t* act;            // MPC: active-set words [count][words]
  const int* status;              // MPC: [count]
  unsigned char* guess;           // MPC: next warm start [count][n]
};

struct NNLayer {                  // one layer of one network
  const float* W;                 // [K][N] (Keras kernel layout)
  const float* bias;              // [N] or null (output layer of a structured network)
  int K, N, row0, rows, last;
};

// y = v^T M for a row-major M (rows x cols) and v in LDS: thread c owns column c (consecutive lanes, consecutive doubles)
__device__ __forceinline__ double colsum(const double* __restrict__ M, int rows, int cols, const double* v, int c) {
  double a = 0.0;
  for (int j = 0; j < rows; ++j) a += M[(size_t)j * cols + c] * v[j];
  return a;
}

__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = CL_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// ---- every instance to the shared initial values (nnmpc_cl_reset)
__global__ __launch_bounds__(CL_THREADS) void cl_reset_k(int nx, int na, int nu, const double* __restrict__ x0,
                                                          const double* __restrict__ xhat0, const double* __restrict__ uprev0,
                                                          double* __restrict__ x, double* __restrict__ xhat, double* __restrict__ uprev,
                                                          double* __restrict__ avg) {
  const int i = blockIdx.x, tid = threadIdx.x;
  for (int k = tid; k < nx; k += CL_THREADS) x[(size_t)i * nx + k] = x0[k];
  for (int k = tid; k < na; k += CL_THREADS) xhat[(size_t)i * na + k] = xhat0[k];
  for (int k = tid; k < nu; k += CL_THREADS) uprev[(size_t)i * nu + k] = uprev0[k];
  if (tid == 0) avg[i] = 0.0;
}

// ---- start of a call: after a reset y_0 = C x0 + sigma o v_0 (LinearPlantSimulator.__init__, :87-100) or the caller's y0; row 0
// of the records
__global__ __launch_bounds__(CL_THREADS) void cl_begin_k(int fresh, int nx, int na, int ny, const double* __restrict__ Ct,
                                                          const double* __restrict__ sigma, const double* __restrict__ v0,
                                                          const double* __restrict__ y0,
                                                          const double* __restrict__ x, const double* __restrict__ xhat,
                                                          const double* __restrict__ avg, double* __restrict__ y,
                                                          double* __restrict__ y_rec, double* __restrict__ x_rec,
                                                          double* __restrict__ xhat_rec, double* __restrict__ avg_rec) {
  extern __shared__ double sx[];
  const int i = blockIdx.x, tid = threadIdx.x;
  for (int k = tid; k < nx; k += CL_THREADS) sx[k] = x[(size_t)i * nx + k];
  __syncthreads();
  if (fresh)
    for (int j = tid; j < ny; j += CL_THREADS)
      y[(size_t)i * ny + j] = y0 ? y0[(size_t)i * ny + j] : colsum(Ct, nx, ny, sx, j) + sigma[j] * v0[(size_t)i * ny + j];
  __syncthreads();
  if (y_rec) for (int j = tid; j < ny; j += CL_THREADS) y_rec[(size_t)i * ny + j] = y[(size_t)i * ny + j];
  if (x_rec) for (int k = tid; k < nx; k += CL_THREADS) x_rec[(size_t)i * nx + k] = sx[k];
  if (xhat_rec) for (int k = tid; k < na; k += CL_THREADS) xhat_rec[(size_t)i * na + k] = xhat[(size_t)i * na + k];
  if (avg_rec && tid == 0) avg_rec[i] = avg[i];
}

// ---- step part 1: filter (KalmanFilter.solve, :108-112) and the reduction of the target problem (target.ReducedTargetProblem)
struct FilterArgs {
  int nx, nu, ny, nd, nz, na, nbv, T;
  const double *Aat, *Bat, *Cat, *Lt;           // transposes: Aaug' (na x na), Baug' (nu x na), Caug' (na x ny), L' (ny x na)
  const double *tbt, *Qbt, *Qyt, *q0, *Cdt, *Ebt; // tb' ((ny + nd) x nbv), Qb' (nbv x nu), Qy' (ny x nu), Cd' (nd x ny), Eb' (nbv x nz)
};
__global__ __launch_bounds__(CL_THREADS) void cl_filter_k(FilterArgs a, int t, const int* __restrict__ scen,
                                                           const double* __restrict__ sp, double* __restrict__ xhat,
                                                           const double* __restrict__ uprev, const double* __restrict__ y,
                                                           double* __restrict__ b, double* __restrict__ q, double* __restrict__ e) {
  extern __shared__ double sm[];
  const int i = blockIdx.x, tid = threadIdx.x;
  const int na = a.na, nu = a.nu, ny = a.ny, nd = a.nd, nx = a.nx, nbv = a.nbv;
  double* z = sm;                    // [na]  xhat
  double* up = z + na;               // [nu]
  double* xp = up + nu;              // [na]
  double* r = xp + na;               // [ny]  innovation, then ysp - Cd dhat
  double* bin = r + ny;              // [ny + nd]  [ysp; dhat]
  double* bv = bin + ny + nd;        // [nbv]
  const double* ysp = sp + ((size_t)scen[i] * a.T + t) * ny;
  for (int k = tid; k < na; k += CL_THREADS) z[k] = xhat[(size_t)i * na + k];
  for (int k = tid; k < nu; k += CL_THREADS) up[k] = uprev[(size_t)i * nu + k];
  __syncthreads();
  for (int k = tid; k < na; k += CL_THREADS) xp[k] = colsum(a.Aat, na, na, z, k) + colsum(a.Bat, nu, na, up, k);
  __syncthreads();
  for (int j = tid; j < ny; j += CL_THREADS) r[j] = y[(size_t)i * ny + j] - colsum(a.Cat, na, ny, xp, j);
  __syncthreads();
  for (int k = tid; k < na; k += CL_THREADS) {
    const double v = xp[k] + colsum(a.Lt, ny, na, r, k);
    xhat[(size_t)i * na + k] = v;
    if (k >= nx) bin[ny + k - nx] = v;
  }
  for (int j = tid; j < ny; j += CL_THREADS) bin[j] = ysp[j];
  __syncthreads();
  for (int m = tid; m < nbv; m += CL_THREADS) {
    const double v = colsum(a.tbt, ny + nd, nbv, bin, m);
    bv[m] = v;
    b[(size_t)i * nbv + m] = v;
  }
  for (int j = tid; j < ny; j += CL_THREADS) r[j] = bin[j] - colsum(a.Cdt, nd, ny, bin + ny, j);
  __syncthreads();
  for (int k = tid; k < nu; k += CL_THREADS) q[(size_t)i * nu + k] = (colsum(a.Qbt, nbv, nu, bv, k) + colsum(a.Qyt, ny, nu, r, k)) + a.q0[k];
  for (int k = tid; k < a.nz; k += CL_THREADS) e[(size_t)i * a.nz + k] = colsum(a.Ebt, nbv, a.nz, bv, k);
}

// ---- step part 2: xs = Xb b + Xu us and each kind's controller input
struct ExpandArgs {
  int nx, nu, na, nbv, ldA;
  const double *Xbt, *Xut, *ulb, *uub;          // Xb' (nbv x nx), Xu' (nu x nx)
};
__global__ __launch_bounds__(CL_THREADS) void cl_expand_k(ExpandArgs a, const int* __restrict__ inst_slot, const SlotDev* __restrict__ slots,
                                                           const int* __restrict__ nn_row, const double* __restrict__ b,
                                                           const double* __restrict__ us, const double* __restrict__ xhat,
                                                           const double* __restrict__ uprev, double* __restrict__ xs,
                                                           double* __restrict__ qx0, double* __restrict__ lb, double* __restrict__ ub,
                                                           double* __restrict__ ctl_u, float* __restrict__ act) {
  extern __shared__ double sm[];
  const int i = blockIdx.x, tid = threadIdx.x;
  const int nx = a.nx, nu = a.nu, nbv = a.nbv;
  double* bv = sm;                   // [nbv]
  double* su = bv + nbv;             // [nu]  us
  double* zz = su + nu;              // [nx + nu]  [xhat - xs; uprev - us]
  double* xsv = zz + nx + nu;        // [nx]
  for (int m = tid; m < nbv; m += CL_THREADS) bv[m] = b[(size_t)i * nbv + m];
  for (int k = tid; k < nu; k += CL_THREADS) su[k] = us[(size_t)i * nu + k];
  __syncthreads();
  for (int k = tid; k < nx; k += CL_THREADS) {
    const double v = colsum(a.Xbt, nbv, nx, bv, k) + colsum(a.Xut, nu, nx, su, k);
    xsv[k] = v;
    xs[(size_t)i * nx + k] = v;
    zz[k] = xhat[(size_t)i * a.na + k] - v;
  }
  for (int k = tid; k < nu; k += CL_THREADS) zz[nx + k] = uprev[(size_t)i * nu + k] - su[k];
  __syncthreads();
  const SlotDev& s = slots[inst_slot[i]];
  if (s.kind == NNMPC_CL_MPC) {                          // get_control_sequence (:682-689)
    for (int k = tid; k < nx + nu; k += CL_THREADS) qx0[(size_t)i * (nx + nu) + k] = zz[k];
    for (int k = tid; k < nu; k += CL_THREADS) {
      lb[(size_t)i * nu + k] = a.ulb[k] - su[k];
      ub[(size_t)i * nu + k] = a.uub[k] - su[k];
    }
  } else if (s.kind == NNMPC_CL_SATDLQR) {               // Kaug [x^ - xs; uprev - us] + us (:1003)
    for (int k = tid; k < nu; k += CL_THREADS) ctl_u[(size_t)i * nu + k] = colsum(s.Kt, nx + nu, nu, zz, k) + su[k];
  } else if (s.kind == NNMPC_CL_US) {
    for (int k = tid; k < nu; k += CL_THREADS) ctl_u[(size_t)i * nu + k] = su[k];
  } else if (s.kind == NNMPC_CL_NN_UNSTD) {              // the one row [x^, (uprev), xs^, us] of an unstructured network
    const int wu = s.with_uprev, o2 = nx + (wu ? nu : 0);
    float* d1 = act + (size_t)nn_row[i] * a.ldA;
    for (int k = tid; k < nx; k += CL_THREADS) {
      const double sc = s.xscale[k];
      d1[k] = (float)(xhat[(size_t)i * a.na + k] / sc); d1[o2 + k] = (float)(xsv[k] / sc);
    }
    for (int k = tid; k < nu; k += CL_THREADS) {
      d1[o2 + nx + k] = (float)su[k];
      if (wu) d1[nx + k] = (float)uprev[(size_t)i * nu + k];
    }
  } else {                                               // NN rows: pass 1 [x^, (uprev), xs^, us], pass 2 [xs^, (us), xs^, us]
    const int wu = s.with_uprev, o2 = nx + (wu ? nu : 0);
    float* d1 = act + (size_t)nn_row[i] * a.ldA;
    float* d2 = act + (size_t)(nn_row[i] + s.count) * a.ldA;
    for (int k = tid; k < nx; k += CL_THREADS) {
      const double sc = s.xscale[k];
      const float xv = (float)(xhat[(size_t)i * a.na + k] / sc), sv = (float)(xsv[k] / sc);
      d1[k] = xv; d1[o2 + k] = sv;
      d2[k] = sv; d2[o2 + k] = sv;
    }
    for (int k = tid; k < nu; k += CL_THREADS) {
      const float uv = (float)su[k];
      d1[o2 + nx + k] = uv; d2[o2 + nx + k] = uv;
      if (wu) { d1[nx + k] = (float)uprev[(size_t)i * nu + k]; d2[nx + k] = uv; }
    }
  }
}

// ---- grouped structured-NN layer: one launch per layer index for ALL networks.  Workgroup = (network, 64 output columns);
// the 4 waves take 4 contiguous K slices, every thread one column and NN_RB rows in registers, the activation rows in LDS.
// A row's sum runs over k in a fixed order inside each slice and the slices are added in a fixed order: its value does not
// depend on how many rows or networks share the launch.  Bias + ReLU fused; the output layer writes o (rows x nu) for cl_post_k:
// v itself for a structured network (it has no head bias), v + bias for an unstructured one.
__global__ __launch_bounds__(256) void cl_nn_layer_k(const NNLayer* __restrict__ desc, const int2* __restrict__ tiles,
                                                     const float* __restrict__ in, float* __restrict__ out, float* __restrict__ o,
                                                     int ldA, int nu) {
  extern __shared__ float sa[];                          // [NN_RB][K]
  __shared__ float red[NN_KS - 1][NN_RB][64];
  const int2 tl = tiles[blockIdx.x];
  const NNLayer d = desc[tl.x];
  const int lane = threadIdx.x & 63, ks = threadIdx.x >> 6;
  const int col = tl.y + lane, K = d.K, N = d.N;
  const int kc = (K + NN_KS - 1) / NN_KS, k0 = ks * kc, k1 = min(K, k0 + kc);
  for (int r0 = 0; r0 < d.rows; r0 += NN_RB) {
    const int nr = min(NN_RB, d.rows - r0);
    __syncthreads();
    for (int idx = threadIdx.x; idx < NN_RB * K; idx += 256) {
      const int r = idx / K, k = idx - r * K;
      sa[idx] = r < nr ? in[(size_t)(d.row0 + r0 + r) * ldA + k] : 0.f;
    }
    __syncthreads();
    float acc[NN_RB];
#pragma unroll
    for (int r = 0; r < NN_RB; ++r) acc[r] = 0.f;
    if (col < N) {
      const float* w = d.W + col;
#pragma unroll 8
      for (int k = k0; k < k1; ++k) {
        const float wv = w[(size_t)k * N];
#pragma unroll
        for (int r = 0; r < NN_RB; ++r) acc[r] = fmaf(sa[r * K + k], wv, acc[r]);
      }
    }
    if (ks > 0) {
#pragma unroll
      for (int r = 0; r < NN_RB; ++r) red[ks - 1][r][lane] = acc[r];
    }
    __syncthreads();
    if (ks == 0 && col < N) {
      const float bb = d.bias ? d.bias[col] : 0.f;
      for (int r = 0; r < nr; ++r) {
        float v = ((acc[r] + red[0][r][lane]) + red[1][r][lane]) + red[2][r][lane];
        const size_t row = (size_t)(d.row0 + r0 + r);
        if (d.last) o[row * nu + col] = d.bias ? v + bb : v;
        else out[row * ldA + col] = __builtin_elementwise_maximum(v + bb, 0.f);   // IEEE 754-2019 maximum: a NaN stays a NaN (fmaxf returns 0)
      }
    }
  }
}

// ---- step part 3: the move, the stage cost and its running mean (:691-701), the plant step (:88-93), records, MPC warm start
struct PostArgs {
  int nx, nu, ny, nd, na, T;
  const double *At, *Bt, *Bpt, *Ct;             // A' (nx x nx), B' (nu x nx), Bp' (nd x nx), C' (nx x ny)
  const double *Qaug, *Raug, *Maug, *ulb, *uub, *sigma;
  int nonlinear;                                // 1: the plant step is cl_cstrs_k's (x, y, their records are left to it)
};
struct PostRec {
  double *y, *x, *xhat, *u, *xs, *us, *avg;     // this step's rows (u/xs/us: row t, the others row t + 1), may be null
  int *tst, *rst;
};
__global__ __launch_bounds__(CL_THREADS) void cl_post_k(PostArgs a, int t, int tglob, const int* __restrict__ inst_slot,
                                                         const SlotDev* __restrict__ slots, const int* __restrict__ nn_row,
                                                         const int* __restrict__ scen, const double* __restrict__ dist,
                                                         const double* __restrict__ vnext, const float* __restrict__ o,
                                                         const double* __restrict__ ctl_u, const double* __restrict__ us,
                                                         const double* __restrict__ xs, const int* __restrict__ tstat,
                                                         double* __restrict__ x, const double* __restrict__ xhat,
                                                         double* __restrict__ uprev, double* __restrict__ y, double* __restrict__ avg,
                                                         PostRec rec) {
  extern __shared__ double sm[];
  const int i = blockIdx.x, tid = threadIdx.x;
  const int nx = a.nx, nu = a.nu, ny = a.ny, nd = a.nd, nz = nx + nu;
  double* z = sm;                    // [nx + nu]
  double* w = z + nz;                // [nu]  u - us
  double* pz = w + nu;               // [nx + nu + nd]  [x; u; p]
  double* xn = pz + nx + nu + nd;    // [nx]
  double* red = xn + nx;             // [CL_THREADS]
  const SlotDev& s = slots[inst_slot[i]];
  const int li = i - s.base;
  for (int k = tid; k < nx; k += CL_THREADS) {
    z[k] = xhat[(size_t)i * a.na + k] - xs[(size_t)i * nx + k];
    pz[k] = x[(size_t)i * nx + k];
  }
  for (int k = tid; k < nu; k += CL_THREADS) {
    const double sk = us[(size_t)i * nu + k];
    z[nx + k] = uprev[(size_t)i * nu + k] - sk;
    double u;
    if (s.kind == NNMPC_CL_MPC) u = s.first[(size_t)li * nu + k] + sk;
    else if (s.kind == NNMPC_CL_NN) {
      const int r1 = nn_row[i], r2 = r1 + s.count;
      u = sk + ((double)o[(size_t)r1 * nu + k] - (double)o[(size_t)r2 * nu + k]);
    } else if (s.kind == NNMPC_CL_NN_UNSTD) u = (double)o[(size_t)nn_row[i] * nu + k];
    else u = ctl_u[(size_t)i * nu + k];
    if (s.kind == NNMPC_CL_NN || s.kind == NNMPC_CL_NN_UNSTD || s.kind == NNMPC_CL_SATDLQR) {   // _clip_control_input
      u = u > a.uub[k] ? a.uub[k] : u;
      u = u < a.ulb[k] ? a.ulb[k] : u;
    }
    w[k] = u - sk;
    pz[nx + k] = u;
    if (rec.u) rec.u[(size_t)i * nu + k] = u;
    if (rec.us) rec.us[(size_t)i * nu + k] = sk;
  }
  const int sc = scen[i];
  for (int k = tid; k < nd; k += CL_THREADS) pz[nx + nu + k] = dist[((size_t)sc * a.T + t) * nd + k];
  __syncthreads();
  // ell = z'Qaug z + w'Raug w + z'Maug w + w'Maug'z
  double part = 0.0;
  for (int k = tid; k < nz; k += CL_THREADS) {
    double qz = 0.0, mw = 0.0;
    for (int j = 0; j < nz; ++j) qz += a.Qaug[(size_t)j * nz + k] * z[j];
    for (int j = 0; j < nu; ++j) mw += a.Maug[(size_t)k * nu + j] * w[j];
    part += z[k] * qz + z[k] * mw;
  }
  for (int k = tid; k < nu; k += CL_THREADS) {
    double rw = 0.0, mz = 0.0;
    for (int j = 0; j < nu; ++j) rw += a.Raug[(size_t)j * nu + k] * w[j];
    for (int j = 0; j < nz; ++j) mz += a.Maug[(size_t)j * nu + k] * z[j];
    part += w[k] * rw + w[k] * mz;
  }
  const double ell = block_sum(part, red);
  if (a.nonlinear) {
    for (int k = tid; k < nu; k += CL_THREADS) uprev[(size_t)i * nu + k] = pz[nx + k];
  } else {
  // plant: x+ = (A x + B u) + Bp p
  for (int k = tid; k < nx; k += CL_THREADS) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int j = 0; j < nx; ++j) a0 += a.At[(size_t)j * nx + k] * pz[j];
    for (int j = 0; j < nu; ++j) a1 += a.Bt[(size_t)j * nx + k] * pz[nx + j];
    for (int j = 0; j < nd; ++j) a2 += a.Bpt[(size_t)j * nx + k] * pz[nx + nu + j];
    const double v = (a0 + a1) + a2;
    xn[k] = v;
    x[(size_t)i * nx + k] = v;
    if (rec.x) rec.x[(size_t)i * nx + k] = v;
  }
  for (int k = tid; k < nu; k += CL_THREADS) uprev[(size_t)i * nu + k] = pz[nx + k];
  __syncthreads();
  for (int j = tid; j < ny; j += CL_THREADS) {
    const double v = colsum(a.Ct, nx, ny, xn, j) + a.sigma[j] * vnext[(size_t)i * ny + j];
    y[(size_t)i * ny + j] = v;
    if (rec.y) rec.y[(size_t)i * ny + j] = v;
  }
  }
  if (rec.xs) for (int k = tid; k < nx; k += CL_THREADS) rec.xs[(size_t)i * nx + k] = xs[(size_t)i * nx + k];
  if (rec.xhat) for (int k = tid; k < a.na; k += CL_THREADS) rec.xhat[(size_t)i * a.na + k] = xhat[(size_t)i * a.na + k];
  if (tid == 0) {
    const double m = (avg[i] * (double)tglob + ell) / (double)(tglob + 1);
    avg[i] = m;
    if (rec.avg) rec.avg[i] = m;
    if (rec.tst) rec.tst[i] = tstat[i];
    if (rec.rst) rec.rst[i] = s.kind == NNMPC_CL_MPC ? s.status[li] : 0;
  }
  if (s.kind == NNMPC_CL_MPC) {                          // next warm start: this step's set shifted by one stage (chain_post_k)
    const uint32_t* aw = s.act + (size_t)li * s.words;
    for (int r = tid; r < s.n; r += CL_THREADS) {
      const int rs = r + nu < s.n ? r + nu : r;
      const int k = rs / nu, j = rs - k * nu;
      const int bu = k * 2 * nu + j, bl = bu + nu;
      const int su_ = (aw[bu >> 5] >> (bu & 31)) & 1u, sl = (aw[bl >> 5] >> (bl & 31)) & 1u;
      s.guess[(size_t)li * s.n + r] = (unsigned char)(su_ ? 1 : (sl ? 2 : 0));
    }
  }
}

// ---- the CSTRs-with-flash plant (NNMPC_CL_PLANT_CSTRS_FLASH): classical RK4, a fixed number of substeps per sample, fp64,
// the tableau and operation order of nonlinearMPC.DiscreteSimulator / cstrs_parameters._rhs.  One lane per instance: the
// 12 states, the accumulator and the stage input stay in registers; the loop counts are kernel arguments, never data.
struct CstrsPar { double c[NNMPC_CSTRS_NPAR]; };
enum { P_aA, P_aB, P_aC, P_rho, P_Cp, P_Ar, P_Am, P_Ab, P_kr, P_km, P_kb, P_dH1, P_dH2, P_EbyR, P_k1, P_k2, P_Td,
       P_XS = 17, P_US = 29, P_PS = 35, P_USC = 40, P_PSC = 46 };

// Constant reciprocals of the right-hand side, formed once per flow map (outside the substep loop)
struct CstrsInv { double rA, mA, bA, cp; };

// f (12) at the deviation state z; U (6), P (5) absolute.  Shared subexpressions once: 2 exponentials, 3 square roots, the
// vapour fractions (one reciprocal of their denominator), the reciprocal hold-ups and temperatures: 6 fp64 reciprocals per
// evaluation, the constant divisors are multiplications by CstrsInv.  A level <= 0 gives NaN (sqrt) or inf (1 / hold-up),
// as numpy does.
__device__ __forceinline__ void cstrs_rhs(const CstrsPar& q, const CstrsInv& v, const double* z, const double* U, const double* P,
                                          double* f) {
  const double* c = q.c;
  const double Hr = z[0] + c[P_XS + 0], xAr = z[1] + c[P_XS + 1], xBr = z[2] + c[P_XS + 2], Tr = z[3] + c[P_XS + 3];
  const double Hm = z[4] + c[P_XS + 4], xAm = z[5] + c[P_XS + 5], xBm = z[6] + c[P_XS + 6], Tm = z[7] + c[P_XS + 7];
  const double Hb = z[8] + c[P_XS + 8], xAb = z[9] + c[P_XS + 9], xBb = z[10] + c[P_XS + 10], Tb = z[11] + c[P_XS + 11];
  const double F0 = U[0], Qr = U[1], F1 = U[2], Qm = U[3], D = U[4], Qb = U[5];
  const double xA0 = P[0], xB0 = P[1], xA1 = P[2], xB1 = P[3], T0 = P[4];
  const double rho = c[P_rho];
  const double ivden = 1.0 / (c[P_aA] * xAb + c[P_aB] * xBb + c[P_aC] * (1.0 - xAb - xBb));
  const double xAd = c[P_aA] * xAb * ivden, xBd = c[P_aB] * xBb * ivden;
  const double Fr = c[P_kr] * sqrt(Hr), Fm = c[P_km] * sqrt(Hm), Fb = c[P_kb] * sqrt(Hb);
  const double Fp = 0.01 * D;
  const double er = exp(-c[P_EbyR] * (1.0 / Tr)), em = exp(-c[P_EbyR] * (1.0 / Tm));
  const double k1r = c[P_k1] * er, k2r = c[P_k2] * er, k1m = c[P_k1] * em, k2m = c[P_k2] * em;
  const double dH1 = c[P_dH1], dH2 = c[P_dH2], Td = c[P_Td];
  const double imr = 1.0 / (rho * c[P_Ar] * Hr), imm = 1.0 / (rho * c[P_Am] * Hm), imb = 1.0 / (rho * c[P_Ab] * Hb);
  f[0] = (F0 + D - Fr) * v.rA;
  f[1] = (F0 * (xA0 - xAr) + D * (xAd - xAr)) * imr - k1r * xAr;
  f[2] = (F0 * (xB0 - xBr) + D * (xBd - xBr)) * imr + k1r * xAr - k2r * xBr;
  f[3] = (F0 * (T0 - Tr) + D * (Td - Tr)) * imr - (k1r * xAr * dH1 + k2r * xBr * dH2) * v.cp + Qr * imr * v.cp;
  f[4] = (Fr + F1 - Fm) * v.mA;
  f[5] = (Fr * (xAr - xAm) + F1 * (xA1 - xAm)) * imm - k1m * xAm;
  f[6] = (Fr * (xBr - xBm) + F1 * (xB1 - xBm)) * imm + k1m * xAm - k2m * xBm;
  f[7] = (Fr * (Tr - Tm) + F1 * (T0 - Tm)) * imm - (k1m * xAm * dH1 + k2m * xBm * dH2) * v.cp + Qm * imm * v.cp;
  f[8] = (Fm - Fb - D - Fp) * v.bA;
  f[9] = (Fm * (xAm - xAb) - (D + Fp) * (xAd - xAb)) * imb;
  f[10] = (Fm * (xBm - xBb) - (D + Fp) * (xBd - xBb)) * imb;
  f[11] = Fm * (Tm - Tb) * imb + Qb * imb * v.cp;
}

// x (12, deviation) <- Phi(x, u, p) over one sample; u (6), p (5) scaled deviations
__device__ __forceinline__ void cstrs_flow(const CstrsPar& q, double h, int substeps, double* x, const double* u, const double* p) {
  double U[6], P[5], k[12], acc[12], z[12];
#pragma unroll
  for (int j = 0; j < 6; ++j) U[j] = u[j] * q.c[P_USC + j] + q.c[P_US + j];
#pragma unroll
  for (int j = 0; j < 5; ++j) P[j] = p[j] * q.c[P_PSC + j] + q.c[P_PS + j];
  const double h2 = 0.5 * h, h6 = h / 6.0;
  const CstrsInv v{1.0 / (q.c[P_rho] * q.c[P_Ar]), 1.0 / (q.c[P_rho] * q.c[P_Am]), 1.0 / (q.c[P_rho] * q.c[P_Ab]), 1.0 / q.c[P_Cp]};
  for (int s = 0; s < substeps; ++s) {
    cstrs_rhs(q, v, x, U, P, k);
#pragma unroll
    for (int j = 0; j < 12; ++j) { acc[j] = k[j]; z[j] = x[j] + h2 * k[j]; }
    cstrs_rhs(q, v, z, U, P, k);
#pragma unroll
    for (int j = 0; j < 12; ++j) { acc[j] = acc[j] + 2.0 * k[j]; z[j] = x[j] + h2 * k[j]; }
    cstrs_rhs(q, v, z, U, P, k);
#pragma unroll
    for (int j = 0; j < 12; ++j) { acc[j] = acc[j] + 2.0 * k[j]; z[j] = x[j] + h * k[j]; }
    cstrs_rhs(q, v, z, U, P, k);
#pragma unroll
    for (int j = 0; j < 12; ++j) x[j] = x[j] + h6 * (acc[j] + k[j]);
  }
}

constexpr int CSTRS_THREADS = 64;

// batched flow map (nnmpc_cstrs_flow): instance i = thread
__global__ __launch_bounds__(CSTRS_THREADS) void cstrs_flow_k(CstrsPar q, double h, int substeps, int nb, const double* __restrict__ x,
                                                              const double* __restrict__ u, const double* __restrict__ p,
                                                              double* __restrict__ xo) {
  const int i = blockIdx.x * CSTRS_THREADS + threadIdx.x;
  if (i >= nb) return;
  double xv[12], uv[6], pv[5];
#pragma unroll
  for (int j = 0; j < 12; ++j) xv[j] = x[(size_t)i * 12 + j];
#pragma unroll
  for (int j = 0; j < 6; ++j) uv[j] = u[(size_t)i * 6 + j];
#pragma unroll
  for (int j = 0; j < 5; ++j) pv[j] = p[(size_t)i * 5 + j];
  cstrs_flow(q, h, substeps, xv, uv, pv);
#pragma unroll
  for (int j = 0; j < 12; ++j) xo[(size_t)i * 12 + j] = xv[j];
}

// step part 4 (nonlinear plant): x = Phi(x, u_t, p_t) with u_t = uprev (cl_post_k wrote it), y_{t+1} = C x + sigma o v_{t+1}
__global__ __launch_bounds__(CSTRS_THREADS) void cl_cstrs_k(CstrsPar q, double h, int substeps, int nb, int ny, int T, int t,
                                                            const int* __restrict__ scen, const double* __restrict__ dist,
                                                            const double* __restrict__ uprev, const double* __restrict__ Ct,
                                                            const double* __restrict__ sigma, const double* __restrict__ vnext,
                                                            double* __restrict__ x, double* __restrict__ y,
                                                            double* __restrict__ x_rec, double* __restrict__ y_rec) {
  const int i = blockIdx.x * CSTRS_THREADS + threadIdx.x;
  if (i >= nb) return;
  double xv[12], uv[6], pv[5];
#pragma unroll
  for (int j = 0; j < 12; ++j) xv[j] = x[(size_t)i * 12 + j];
#pragma unroll
  for (int j = 0; j < 6; ++j) uv[j] = uprev[(size_t)i * 6 + j];
  const double* pt = dist + ((size_t)scen[i] * T + t) * 5;
#pragma unroll
  for (int j = 0; j < 5; ++j) pv[j] = pt[j];
  cstrs_flow(q, h, substeps, xv, uv, pv);
#pragma unroll
  for (int j = 0; j < 12; ++j) {
    x[(size_t)i * 12 + j] = xv[j];
    if (x_rec) x_rec[(size_t)i * 12 + j] = xv[j];
  }
  for (int j = 0; j < ny; ++j) {                         // colsum order of cl_post_k's linear measurement
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < 12; ++k) a += Ct[(size_t)k * ny + j] * xv[k];
    const double v = a + sigma[j] * vnext[(size_t)i * ny + j];
    y[(size_t)i * ny + j] = v;
    if (y_rec) y_rec[(size_t)i * ny + j] = v;
  }
}

// the parameter block of nnmpc_cl_set_plant / nnmpc_cstrs_flow: finite, positive where a physical quantity must be
int cstrs_check(const double* par, int32_t npar, double sample_time, int32_t substeps, CstrsPar* q, const char* who) {
  if (!par || npar != NNMPC_CSTRS_NPAR || !(sample_time > 0.0) || !(sample_time < 1e300) || substeps < 1 || substeps > 4096) {
    set_error("%s: needs %d parameters, sample_time > 0 and 1 <= substeps <= 4096 (got npar=%d, sample_time=%g, substeps=%d)",
              who, NNMPC_CSTRS_NPAR, npar, sample_time, substeps);
    return NNMPC_EINVAL;
  }
  for (int j = 0; j < npar; ++j)
    if (!(fabs(par[j]) <= 1.79e308)) { set_error("%s: parameter %d is not finite", who, j); return NNMPC_EINVAL; }
  const int pos[] = {P_rho, P_Cp, P_Ar, P_Am, P_Ab};
  for (int j : pos)
    if (!(par[j] > 0.0)) { set_error("%s: parameter %d (density, heat capacity, areas) must be > 0", who, j); return NNMPC_EINVAL; }
  for (int j = 0; j < npar; ++j) q->c[j] = par[j];
  return NNMPC_OK;
}

std::vector<double> transpose(const double* M, int rows, int cols) {
  std::vector<double> t((size_t)rows * cols);
  for (int i = 0; i < rows; ++i)
    for (int j = 0; j < cols; ++j) t[(size_t)j * rows + i] = M[(size_t)i * cols + j];
  return t;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------
struct nnmpc_cl {
  int device = 0, nx = 0, nu = 0, ny = 0, nd = 0, nz = 0, na = 0, nbv = 0, nb = 0, nslots = 0;
  nnmpc_ts* ts = nullptr;
  std::vector<int> kind, base, count;               // per slot (host)
  std::vector<nnmpc_qp*> qp;
  std::vector<bool> have_guess;
  std::vector<SlotDev> sd;                          // host copy of the slot table
  SlotDev* slots_d = nullptr;
  int* inst_slot = nullptr;
  int* nn_row = nullptr;
  // shared matrices (device)
  double *At, *Bt, *Bpt, *Ct, *Aat, *Bat, *Cat, *Lt, *tbt, *Qbt, *Qyt, *q0, *Cdt, *Ebt, *Xbt, *Xut, *Qaug, *Raug, *Maug;
  double *ulb, *uub, *x0, *xhat0, *uprev0;
  // instance state and step workspace
  double *x, *xhat, *uprev, *y, *avg, *b, *q, *e, *us, *xs, *qx0, *lb, *ub, *first, *ctl_u;
  int *tstat, *rstat;
  // grouped NN
  int nn_rows = 0, ldA = 0, nn_layers = 0;
  float *act[2] = {nullptr, nullptr}, *o = nullptr;
  NNLayer* desc_d = nullptr;
  int2* tiles_d = nullptr;
  std::vector<int> tile_off, tile_cnt;              // per layer index
  int maxK = 0;
  bool fresh = true;
  int64_t tglob = 0;
  hipStream_t stream = nullptr;
  double total_ms = 0.0, phase_ms[6] = {0, 0, 0, 0, 0, 0};
  int plant = NNMPC_CL_PLANT_LINEAR;                // nnmpc_cl_set_plant
  CstrsPar cstrs = {};
  double plant_h = 0.0, plant_ms = 0.0;
  int plant_substeps = 0;
  std::vector<double> slot_ms;                      // [T][nslots] of the last run
  int last_T = 0;
  DevRes res{15};                                   // owns all of it; its slots: staging of host-pointer runs; its pool: the phase events
};

extern "C" {

int nnmpc_cl_create(nnmpc_cl** out, const nnmpc_cl_model* m, nnmpc_ts* ts, int32_t nslots, const nnmpc_cl_slot* slots,
                    int32_t nb, const int32_t* inst_slot) {
  if (!out || !m || !ts || nslots <= 0 || !slots || nb <= 0 || !inst_slot) {
    set_error("nnmpc_cl_create: bad arguments (nslots=%d nb=%d)", nslots, nb);
    return NNMPC_EINVAL;
  }
  const int nx = m->nx, nu = m->nu, ny = m->ny, nd = m->nd, nz = m->nz;
  if (nx <= 0 || nu <= 0 || ny <= 0 || nd < 0 || nz < 0) { set_error("nnmpc_cl_create: bad sizes nx=%d nu=%d ny=%d nd=%d nz=%d", nx, nu, ny, nd, nz); return NNMPC_EINVAL; }
  const double* need[] = {m->A, m->B, m->C, m->Aaug, m->Baug, m->Caug, m->L, m->tb, m->Qb, m->Qy, m->q0, m->Xb, m->Xu,
                          m->Qaug, m->Raug, m->Maug, m->ulb, m->uub, m->x0, m->xhat0, m->uprev0};
  for (const double* p : need) if (!p) { set_error("nnmpc_cl_create: a model matrix is NULL"); return NNMPC_EINVAL; }
  if ((nd && (!m->Bp || !m->Cd)) || (nz && !m->Eb)) { set_error("nnmpc_cl_create: Bp / Cd (nd > 0) or Eb (nz > 0) is NULL"); return NNMPC_EINVAL; }
  int tnu = 0, tnz = 0;
  if (nnmpc_ts_dims_internal(ts, &tnu, &tnz) || tnu != nu || tnz != nz) {
    set_error("nnmpc_cl_create: target handle has nu=%d nz=%d, the model nu=%d nz=%d", tnu, tnz, nu, nz);
    return NNMPC_EINVAL;
  }
  for (int i = 0; i < nb; ++i)
    if (inst_slot[i] < 0 || inst_slot[i] >= nslots || (i && inst_slot[i] < inst_slot[i - 1])) {
      set_error("nnmpc_cl_create: inst_slot[%d] = %d (slots 0..%d, non-decreasing)", i, inst_slot[i], nslots - 1);
      return NNMPC_EINVAL;
    }
  for (int k = 0; k < nslots; ++k) {
    const nnmpc_cl_slot& s = slots[k];
    if (s.kind == NNMPC_CL_MPC) {
      int n = 0, qnu = 0, qna = 0;
      if (!s.qp || nnmpc_qp_dims(s.qp, &n, &qnu, &qna) || qnu != nu || qna != nx + nu) {
        set_error("nnmpc_cl_create: slot %d (MPC) needs a regulator handle with nu=%d n_aug=%d", k, nu, nx + nu);
        return NNMPC_EINVAL;
      }
    } else if (s.kind == NNMPC_CL_NN || s.kind == NNMPC_CL_NN_UNSTD) {
      const bool un = s.kind == NNMPC_CL_NN_UNSTD;
      const int din = 2 * nx + (s.with_uprev ? 2 : 1) * nu;
      if (s.nlayers < 1 || !s.dims || !s.W || !s.b || s.dims[0] != din || s.dims[s.nlayers] != nu) {
        set_error("nnmpc_cl_create: slot %d (NN) needs dims [%d, ..., %d] with weights and biases", k, din, nu);
        return NNMPC_EINVAL;
      }
      for (int l = 0; l < s.nlayers; ++l)
        if (s.dims[l] <= 0 || s.dims[l] > NN_MAXK || s.dims[l + 1] <= 0 || !s.W[l] || ((un || l < s.nlayers - 1) && !s.b[l])) {
          set_error("nnmpc_cl_create: slot %d (NN) layer %d: widths 1..%d, weights and (hidden; unstructured: all) biases required", k, l, NN_MAXK);
          return NNMPC_EINVAL;
        }
    } else if (s.kind == NNMPC_CL_SATDLQR) {
      if (!s.Kaug) { set_error("nnmpc_cl_create: slot %d (SATDLQR) has no Kaug", k); return NNMPC_EINVAL; }
    } else if (s.kind != NNMPC_CL_US) {
      set_error("nnmpc_cl_create: slot %d has unknown kind %d", k, s.kind);
      return NNMPC_EINVAL;
    }
  }
  GUARD_BEGIN
  if (int rc = check_device(__func__)) return rc;
  Building<nnmpc_cl, nnmpc_cl_destroy> guard(new nnmpc_cl());   // released into *out at the end; destroyed on any other way out
  nnmpc_cl* h = guard.get();
  DevRes& res = h->res;
  h->nx = nx; h->nu = nu; h->ny = ny; h->nd = nd; h->nz = nz; h->na = nx + nd; h->nbv = nx + nz; h->nb = nb; h->nslots = nslots;
  h->ts = ts;
  HIPCHK(hipGetDevice(&h->device));
  res.device = h->device;
  if (int rc = res.stream(&h->stream)) return rc;
  const int na = h->na, nbv = h->nbv, nzz = nx + nu;
  // a matrix transposed, or as it is; an absent or empty one is one zero
  auto upT = [&](double** p, const double* M, int r, int c) { return (M && r * c) ? res.upload(p, transpose(M, r, c).data(), (size_t)r * c) : res.alloc(p, 1); };
  auto upD = [&](double** p, const double* M, size_t cnt) { return (M && cnt) ? res.upload(p, M, cnt) : res.alloc(p, 1); };
#define OK_(x) if (int rc = (x)) return rc
#define A_(ptr, cnt) OK_(res.alloc(&(ptr), (size_t)(cnt)))
  OK_(upT(&h->At, m->A, nx, nx)); OK_(upT(&h->Bt, m->B, nx, nu)); OK_(upT(&h->Bpt, m->Bp, nx, nd)); OK_(upT(&h->Ct, m->C, ny, nx));
  OK_(upT(&h->Aat, m->Aaug, na, na)); OK_(upT(&h->Bat, m->Baug, na, nu)); OK_(upT(&h->Cat, m->Caug, ny, na)); OK_(upT(&h->Lt, m->L, na, ny));
  OK_(upT(&h->tbt, m->tb, nbv, ny + nd)); OK_(upT(&h->Qbt, m->Qb, nu, nbv)); OK_(upT(&h->Qyt, m->Qy, nu, ny)); OK_(upD(&h->q0, m->q0, nu));
  OK_(upT(&h->Cdt, m->Cd, ny, nd)); OK_(upT(&h->Ebt, m->Eb, nz, nbv)); OK_(upT(&h->Xbt, m->Xb, nx, nbv)); OK_(upT(&h->Xut, m->Xu, nx, nu));
  OK_(upD(&h->Qaug, m->Qaug, (size_t)nzz * nzz)); OK_(upD(&h->Raug, m->Raug, (size_t)nu * nu)); OK_(upD(&h->Maug, m->Maug, (size_t)nzz * nu));
  OK_(upD(&h->ulb, m->ulb, nu)); OK_(upD(&h->uub, m->uub, nu)); OK_(upD(&h->x0, m->x0, nx)); OK_(upD(&h->xhat0, m->xhat0, na)); OK_(upD(&h->uprev0, m->uprev0, nu));
  A_(h->x, (size_t)nb * nx); A_(h->xhat, (size_t)nb * na); A_(h->uprev, (size_t)nb * nu); A_(h->y, (size_t)nb * ny); A_(h->avg, nb);
  A_(h->b, (size_t)nb * nbv); A_(h->q, (size_t)nb * nu); A_(h->e, (size_t)nb * std::max(nz, 1)); A_(h->us, (size_t)nb * nu);
  A_(h->xs, (size_t)nb * nx); A_(h->qx0, (size_t)nb * nzz); A_(h->lb, (size_t)nb * nu); A_(h->ub, (size_t)nb * nu);
  A_(h->first, (size_t)nb * nu); A_(h->ctl_u, (size_t)nb * nu); A_(h->tstat, nb); A_(h->rstat, nb);
  // slot table and instance ranges
  h->kind.resize(nslots); h->base.assign(nslots, 0); h->count.assign(nslots, 0); h->qp.assign(nslots, nullptr);
  h->have_guess.assign(nslots, false); h->sd.resize(nslots);
  for (int i = 0; i < nb; ++i) h->count[inst_slot[i]]++;
  for (int k = 1; k < nslots; ++k) h->base[k] = h->base[k - 1] + h->count[k - 1];
  std::vector<int> nn_row(nb, 0);
  std::vector<std::vector<NNLayer>> layers(nslots);
  for (int k = 0; k < nslots; ++k) {
    const nnmpc_cl_slot& s = slots[k];
    SlotDev& d = h->sd[k];
    memset(&d, 0, sizeof(d));
    d.kind = s.kind; d.base = h->base[k]; d.count = h->count[k];
    h->kind[k] = s.kind;
    if (s.kind == NNMPC_CL_MPC) {
      int n = 0, qnu = 0, qna = 0;
      nnmpc_qp_dims(s.qp, &n, &qnu, &qna);
      h->qp[k] = s.qp;
      d.n = n; d.words = (2 * n + 31) / 32;
      d.first = h->first + (size_t)d.base * nu;
      d.status = h->rstat + d.base;
      uint32_t* act = nullptr; unsigned char* g = nullptr;
      A_(act, (size_t)std::max(d.count, 1) * d.words);
      A_(g, (size_t)std::max(d.count, 1) * n);
      d.act = act; d.guess = g;
    } else if (s.kind == NNMPC_CL_SATDLQR) {
      double* kt = nullptr;
      OK_(upT(&kt, s.Kaug, nu, nzz));
      d.Kt = kt;
    } else if (s.kind == NNMPC_CL_NN || s.kind == NNMPC_CL_NN_UNSTD) {
      const bool un = s.kind == NNMPC_CL_NN_UNSTD;
      const int rows = un ? d.count : 2 * d.count;       // unstructured: one pass, one row per instance
      d.with_uprev = s.with_uprev ? 1 : 0;
      d.row0 = h->nn_rows;
      std::vector<double> xsc(nx, 1.0);
      if (s.xscale) for (int j = 0; j < nx; ++j) xsc[j] = s.xscale[j];
      double* xd = nullptr;
      OK_(res.upload(&xd, xsc.data(), xsc.size()));
      d.xscale = xd;
      for (int j = 0; j < d.count; ++j) nn_row[d.base + j] = h->nn_rows + j;
      for (int l = 0; l < s.nlayers; ++l) {
        const int K = s.dims[l], N = s.dims[l + 1];
        std::vector<float> wf((size_t)K * N), bf(N, 0.f);
        for (size_t j = 0; j < wf.size(); ++j) wf[j] = (float)s.W[l][j];
        const bool last = l == s.nlayers - 1;
        if (!last || un) for (int j = 0; j < N; ++j) bf[j] = (float)s.b[l][j];
        float *wd = nullptr, *bd = nullptr;
        OK_(res.upload(&wd, wf.data(), wf.size()));
        if (!last || un) OK_(res.upload(&bd, bf.data(), bf.size()));
        layers[k].push_back(NNLayer{wd, bd, K, N, h->nn_rows, rows, last ? 1 : 0});
        h->maxK = std::max(h->maxK, K);
        if (!last) h->ldA = std::max(h->ldA, N);
      }
      h->ldA = std::max(h->ldA, s.dims[0]);
      h->nn_layers = std::max(h->nn_layers, s.nlayers);
      h->nn_rows += rows;
    }
  }
  OK_(res.upload(&h->slots_d, h->sd.data(), h->sd.size()));
  OK_(res.upload(&h->inst_slot, (const int*)inst_slot, (size_t)nb));
  OK_(res.upload(&h->nn_row, nn_row.data(), nn_row.size()));
  if (h->nn_rows) {
    // layer-major descriptor table and the (network, column tile) list of every layer index
    std::vector<NNLayer> desc;
    std::vector<int2> tiles;
    for (int l = 0; l < h->nn_layers; ++l) {
      h->tile_off.push_back((int)tiles.size());
      for (int k = 0; k < nslots; ++k) {
        if ((int)layers[k].size() <= l || h->count[k] == 0) continue;
        const NNLayer& L = layers[k][l];
        const int di = (int)desc.size();
        desc.push_back(L);
        for (int c0 = 0; c0 < L.N; c0 += 64) tiles.push_back(make_int2(di, c0));
      }
      h->tile_cnt.push_back((int)tiles.size() - h->tile_off.back());
    }
    OK_(res.upload(&h->desc_d, desc.data(), desc.size()));
    OK_(res.upload(&h->tiles_d, tiles.data(), tiles.size()));
    A_(h->act[0], (size_t)h->nn_rows * h->ldA); A_(h->act[1], (size_t)h->nn_rows * h->ldA); A_(h->o, (size_t)h->nn_rows * nu);
    HIPCHK(hipFuncSetAttribute((const void*)cl_nn_layer_k, hipFuncAttributeMaxDynamicSharedMemorySize, NN_RB * NN_MAXK * (int)sizeof(float)));
  }
#undef A_
#undef OK_
  if (int rc = nnmpc_cl_reset(h)) return rc;
  *out = guard.release();
  return NNMPC_OK;
  GUARD_END
}

int nnmpc_cl_destroy(nnmpc_cl* h) {
  if (!h) return NNMPC_OK;
  h->res.release();
  delete h;
  return NNMPC_OK;
}

int nnmpc_cl_reset(nnmpc_cl* h) {
  if (!h) { set_error("nnmpc_cl_reset: null handle"); return NNMPC_EINVAL; }
  HIPCHK(hipSetDevice(h->device));
  hipLaunchKernelGGL(cl_reset_k, dim3(h->nb), dim3(CL_THREADS), 0, h->stream, h->nx, h->na, h->nu, h->x0, h->xhat0, h->uprev0,
                     h->x, h->xhat, h->uprev, h->avg);
  HIPCHK(stream_sync(h->stream));
  HIPCHK(hipGetLastError());
  h->fresh = true;
  h->tglob = 0;
  h->have_guess.assign(h->nslots, false);
  return NNMPC_OK;
}

int nnmpc_cl_run(nnmpc_cl* h, int32_t T, int32_t nscen, const double* setpoints, const double* dist, const int32_t* scen,
                 const double* v, const double* sigma, const double* y0, double* y_rec, double* x_rec, double* xhat_rec, double* u_rec,
                 double* xs_rec, double* us_rec, double* avg_rec, int32_t* ts_status, int32_t* reg_status, int32_t ptr_kind) {
  if (!h || T < 0 || nscen <= 0 || !setpoints || (h->nd && !dist) || !scen || !v || !sigma ||
      (ptr_kind != NNMPC_HOST && ptr_kind != NNMPC_DEVICE)) {
    set_error("nnmpc_cl_run: bad arguments");
    return NNMPC_EINVAL;
  }
  if (T == 0) return NNMPC_OK;
  GUARD_BEGIN
  HIPCHK(hipSetDevice(h->device));
  DevRes& res = h->res;
  const int nb = h->nb, nx = h->nx, nu = h->nu, ny = h->ny, nd = h->nd, na = h->na, nbv = h->nbv;
  // scenario indices are checked on the host before anything is launched (device pointers: one copy of nb ints)
  std::vector<int32_t> sc(nb);
  if (ptr_kind == NNMPC_HOST) memcpy(sc.data(), scen, (size_t)nb * 4);
  else HIPCHK(hipMemcpy(sc.data(), scen, (size_t)nb * 4, hipMemcpyDeviceToHost));
  for (int i = 0; i < nb; ++i)
    if (sc[i] < 0 || sc[i] >= nscen) { set_error("nnmpc_cl_run: scen[%d] = %d outside 0..%d", i, sc[i], nscen - 1); return NNMPC_EINVAL; }
  const size_t n_sp = (size_t)nscen * T * ny, n_d = (size_t)nscen * T * nd, n_v = (size_t)(T + 1) * nb * ny;
  const double *sp_d = setpoints, *d_d = dist, *v_d = v, *sig_d = sigma, *y0_d = y0;
  const int* sc_d = scen;
  double* rd[7] = {y_rec, x_rec, xhat_rec, u_rec, xs_rec, us_rec, avg_rec};
  int* rs[2] = {ts_status, reg_status};
  const size_t rsz[7] = {(size_t)(T + 1) * nb * ny, (size_t)(T + 1) * nb * nx, (size_t)(T + 1) * nb * na, (size_t)T * nb * nu,
                         (size_t)T * nb * nx, (size_t)T * nb * nu, (size_t)(T + 1) * nb};
  double* rdd[7];
  int* rsd[2];
  for (int k = 0; k < 7; ++k) rdd[k] = rd[k];
  for (int k = 0; k < 2; ++k) rsd[k] = rs[k];
  if (ptr_kind == NNMPC_HOST) {
    double *a = nullptr, *b = nullptr, *c = nullptr, *s = nullptr;
    int* si = nullptr;
    if (int rc = res.slot(0, &a, n_sp * 8)) return rc;
    if (int rc = res.slot(1, &b, std::max<size_t>(n_d, 1) * 8)) return rc;
    if (int rc = res.slot(2, &c, n_v * 8)) return rc;
    if (int rc = res.slot(3, &s, (size_t)ny * 8)) return rc;
    if (int rc = res.slot(4, &si, (size_t)nb * 4)) return rc;
    double* yy = nullptr;
    if (y0) if (int rc = res.slot(14, &yy, (size_t)nb * ny * 8)) return rc;
    for (int k = 0; k < 7; ++k) if (rd[k]) if (int rc = res.slot(5 + k, &rdd[k], rsz[k] * 8)) return rc;
    for (int k = 0; k < 2; ++k) if (rs[k]) if (int rc = res.slot(12 + k, &rsd[k], (size_t)T * nb * 4)) return rc;
    HIPCHK(hipMemcpy(a, setpoints, n_sp * 8, hipMemcpyHostToDevice));
    if (n_d) HIPCHK(hipMemcpy(b, dist, n_d * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c, v, n_v * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s, sigma, (size_t)ny * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(si, scen, (size_t)nb * 4, hipMemcpyHostToDevice));
    if (y0) HIPCHK(hipMemcpy(yy, y0, (size_t)nb * ny * 8, hipMemcpyHostToDevice));
    sp_d = a; d_d = b; v_d = c; sig_d = s; sc_d = si; y0_d = yy;
  }
  std::vector<int> mpc;
  for (int k = 0; k < h->nslots; ++k) if (h->kind[k] == NNMPC_CL_MPC && h->count[k]) mpc.push_back(k);
  const int nl = h->plant != NNMPC_CL_PLANT_LINEAR ? 1 : 0;
  const int nm = (int)mpc.size(), ne = 7 + nm + nl;     // events per step: start, filter, target, expand, nn, [mpc...], join, post, [plant]
  // phase events of at most CL_EV_BLOCK steps are alive at a time: after each block the stream is drained once and the block's
  // times are added up, so the pool is bounded whatever T is
  const int blk = std::min(T, CL_EV_BLOCK);
  hipEvent_t ev_t0, ev_t1;
  if (int rc = res.pool_event((size_t)blk * ne + 1, &ev_t1)) return rc;
  if (int rc = res.pool_event((size_t)blk * ne, &ev_t0)) return rc;
  hipStream_t s = h->stream;
  FilterArgs fa{nx, nu, ny, nd, h->nz, na, nbv, T, h->Aat, h->Bat, h->Cat, h->Lt, h->tbt, h->Qbt, h->Qyt, h->q0, h->Cdt, h->Ebt};
  ExpandArgs xa{nx, nu, na, nbv, h->ldA, h->Xbt, h->Xut, h->ulb, h->uub};
  PostArgs pa{nx, nu, ny, nd, na, T, h->At, h->Bt, h->Bpt, h->Ct, h->Qaug, h->Raug, h->Maug, h->ulb, h->uub, sig_d, nl};
  const size_t lds_f = (size_t)(2 * na + nu + 2 * ny + nd + nbv) * 8;
  const size_t lds_x = (size_t)(nbv + 2 * nu + 2 * nx) * 8;
  const size_t lds_p = (size_t)(2 * (nx + nu) + nu + nd + nx + CL_THREADS) * 8 + (size_t)nx * 8;
  for (double& p : h->phase_ms) p = 0.0;
  h->plant_ms = 0.0;
  h->slot_ms.assign((size_t)T * h->nslots, 0.0);
  auto el = [&](hipEvent_t a, hipEvent_t b) { float ms = 0.f; hipEventElapsedTime(&ms, a, b); return (double)ms; };
  std::vector<double> ms(nm);
  auto collect = [&](int t0, int t1) {                   // steps [t0, t1) of the current block, stream drained
    for (int t = t0; t < t1; ++t) {
      hipEvent_t* E = res.pool.data() + (size_t)(t - t0) * ne;
      const double f = el(E[0], E[1]), tg = el(E[1], E[2]), xp = el(E[2], E[3]), nn = el(E[3], E[4]);
      double mp = 0.0;
      for (int j = 0; j < nm; ++j) { ms[j] = el(E[3], E[5 + j]); mp = std::max(mp, ms[j]); }
      h->phase_ms[0] += f; h->phase_ms[1] += tg; h->phase_ms[2] += xp; h->phase_ms[3] += nn; h->phase_ms[4] += mp;
      h->phase_ms[5] += el(E[5 + nm], E[6 + nm]);
      if (nl) h->plant_ms += el(E[6 + nm], E[7 + nm]);
      for (int k = 0, j = 0; k < h->nslots; ++k) {
        double v_ = xp;
        if (h->kind[k] == NNMPC_CL_NN || h->kind[k] == NNMPC_CL_NN_UNSTD) v_ = nn;
        else if (h->kind[k] == NNMPC_CL_MPC) v_ = h->count[k] ? ms[j++] : 0.0;
        h->slot_ms[(size_t)t * h->nslots + k] = v_;
      }
    }
  };
  HIPCHK(hipEventRecord(ev_t0, s));
  hipLaunchKernelGGL(cl_begin_k, dim3(nb), dim3(CL_THREADS), (size_t)nx * 8, s, h->fresh ? 1 : 0, nx, na, ny, h->Ct, sig_d, v_d, y0_d,
                     h->x, h->xhat, h->avg, h->y, rdd[0], rdd[1], rdd[2], rdd[6]);
  int tb = 0;                                            // first step of the current event block
  for (int t = 0; t < T; ++t) {
    if (t - tb == blk) {
      HIPCHK(stream_sync(s));
      collect(tb, t);
      tb = t;
    }
    hipEvent_t* E = res.pool.data() + (size_t)(t - tb) * ne;
    hipEventRecord(E[0], s);
    hipLaunchKernelGGL(cl_filter_k, dim3(nb), dim3(CL_THREADS), lds_f, s, fa, t, sc_d, sp_d, h->xhat, h->uprev, h->y, h->b, h->q, h->e);
    hipEventRecord(E[1], s);
    int rc = nnmpc_ts_launch_internal(h->ts, nb, h->q, h->e, h->us, h->tstat, s);
    if (rc) { hipStreamSynchronize(s); return rc; }
    hipEventRecord(E[2], s);
    hipLaunchKernelGGL(cl_expand_k, dim3(nb), dim3(CL_THREADS), lds_x, s, xa, h->inst_slot, h->slots_d, h->nn_row, h->b, h->us,
                       h->xhat, h->uprev, h->xs, h->qx0, h->lb, h->ub, h->ctl_u, h->act[0]);
    hipEventRecord(E[3], s);
    for (int l = 0; l < h->nn_layers; ++l)
      if (h->tile_cnt[l])
        hipLaunchKernelGGL(cl_nn_layer_k, dim3(h->tile_cnt[l]), dim3(256), (size_t)NN_RB * h->maxK * 4, s, h->desc_d,
                           h->tiles_d + h->tile_off[l], h->act[l & 1], h->act[(l + 1) & 1], h->o, h->ldA, nu);
    hipEventRecord(E[4], s);
    for (int j = 0; j < nm; ++j) {                       // the regulator QPs, beside the NN layers
      const int k = mpc[j];
      const SlotDev& d = h->sd[k];
      hipStream_t qs = nnmpc_qp_stream_internal(h->qp[k]);
      HIPCHK(hipStreamWaitEvent(qs, E[3], 0));
      rc = nnmpc_qp_solve_batch_ex(h->qp[k], d.count, h->qx0 + (size_t)d.base * (nx + nu), h->lb + (size_t)d.base * nu,
                                   h->ub + (size_t)d.base * nu, h->have_guess[k] ? d.guess : nullptr, h->first + (size_t)d.base * nu,
                                   const_cast<uint32_t*>(d.act), h->rstat + d.base, nullptr, NNMPC_DEVICE, NNMPC_OUT_FIRST_MOVE);
      if (rc) {
        // half a step done: drain and drop the warm starts (the caller should nnmpc_cl_reset)
        hipStreamSynchronize(s);
        h->have_guess.assign(h->nslots, false);
        return rc;
      }
      HIPCHK(hipEventRecord(E[5 + j], qs));
      HIPCHK(hipStreamWaitEvent(s, E[5 + j], 0));
    }
    hipEventRecord(E[5 + nm], s);
    PostRec pr{rdd[0] ? rdd[0] + (size_t)(t + 1) * nb * ny : nullptr, rdd[1] ? rdd[1] + (size_t)(t + 1) * nb * nx : nullptr,
               rdd[2] ? rdd[2] + (size_t)(t + 1) * nb * na : nullptr, rdd[3] ? rdd[3] + (size_t)t * nb * nu : nullptr,
               rdd[4] ? rdd[4] + (size_t)t * nb * nx : nullptr, rdd[5] ? rdd[5] + (size_t)t * nb * nu : nullptr,
               rdd[6] ? rdd[6] + (size_t)(t + 1) * nb : nullptr, rsd[0] ? rsd[0] + (size_t)t * nb : nullptr,
               rsd[1] ? rsd[1] + (size_t)t * nb : nullptr};
    hipLaunchKernelGGL(cl_post_k, dim3(nb), dim3(CL_THREADS), lds_p, s, pa, t, (int)h->tglob, h->inst_slot, h->slots_d, h->nn_row, sc_d,
                       d_d, v_d + (size_t)(t + 1) * nb * ny, h->o, h->ctl_u, h->us, h->xs, h->tstat, h->x, h->xhat, h->uprev, h->y,
                       h->avg, pr);
    hipEventRecord(E[6 + nm], s);
    if (nl) {
      hipLaunchKernelGGL(cl_cstrs_k, dim3((nb + CSTRS_THREADS - 1) / CSTRS_THREADS), dim3(CSTRS_THREADS), 0, s, h->cstrs, h->plant_h,
                         h->plant_substeps, nb, ny, T, t, sc_d, d_d, h->uprev, h->Ct, sig_d, v_d + (size_t)(t + 1) * nb * ny, h->x,
                         h->y, pr.x, pr.y);
      hipEventRecord(E[7 + nm], s);
    }
    for (int k : mpc) h->have_guess[k] = true;
    h->fresh = false;
    ++h->tglob;
  }
  HIPCHK(hipEventRecord(ev_t1, s));
  HIPCHK(stream_sync(s));
  HIPCHK(hipGetLastError());
  collect(tb, T);
  h->total_ms = el(ev_t0, ev_t1);
  h->last_T = T;
  if (ptr_kind == NNMPC_HOST) {
    for (int k = 0; k < 7; ++k) if (rd[k]) HIPCHK(hipMemcpy(rd[k], rdd[k], rsz[k] * 8, hipMemcpyDeviceToHost));
    for (int k = 0; k < 2; ++k) if (rs[k]) HIPCHK(hipMemcpy(rs[k], rsd[k], (size_t)T * nb * 4, hipMemcpyDeviceToHost));
  }
  return NNMPC_OK;
  GUARD_END
}

int nnmpc_cl_last_ms(nnmpc_cl* h, double* total_ms, double* phase_ms, double* slot_step_ms) {
  if (!h) { set_error("nnmpc_cl_last_ms: null handle"); return NNMPC_EINVAL; }
  if (total_ms) *total_ms = h->total_ms;
  if (phase_ms) for (int k = 0; k < 6; ++k) phase_ms[k] = h->phase_ms[k];
  if (slot_step_ms && !h->slot_ms.empty()) memcpy(slot_step_ms, h->slot_ms.data(), h->slot_ms.size() * 8);
  return NNMPC_OK;
}

int nnmpc_cl_set_plant(nnmpc_cl* h, int32_t kind, const double* par, int32_t npar, double sample_time, int32_t substeps) {
  if (!h) { set_error("nnmpc_cl_set_plant: null handle"); return NNMPC_EINVAL; }
  if (kind == NNMPC_CL_PLANT_LINEAR) { h->plant = kind; return NNMPC_OK; }
  if (kind != NNMPC_CL_PLANT_CSTRS_FLASH) { set_error("nnmpc_cl_set_plant: unknown plant kind %d", kind); return NNMPC_EINVAL; }
  if (h->nx != 12 || h->nu != 6 || h->nd != 5) {
    set_error("nnmpc_cl_set_plant: the CSTRs-with-flash plant needs nx=12 nu=6 nd=5 (handle: nx=%d nu=%d nd=%d)", h->nx, h->nu, h->nd);
    return NNMPC_EINVAL;
  }
  CstrsPar q;
  const int rc = cstrs_check(par, npar, sample_time, substeps, &q, "nnmpc_cl_set_plant");
  if (rc) return rc;
  h->cstrs = q;
  h->plant_h = sample_time / substeps;
  h->plant_substeps = substeps;
  h->plant = kind;
  return NNMPC_OK;
}

int nnmpc_cl_last_plant_ms(nnmpc_cl* h, double* plant_ms) {
  if (!h || !plant_ms) { set_error("nnmpc_cl_last_plant_ms: bad arguments"); return NNMPC_EINVAL; }
  *plant_ms = h->plant_ms;
  return NNMPC_OK;
}

int nnmpc_cstrs_flow(int32_t nb, const double* par, int32_t npar, double sample_time, int32_t substeps, const double* x,
                     const double* u, const double* p, double* x_out, int32_t ptr_kind) {
  if (nb < 0 || (nb && (!x || !u || !p || !x_out)) || (ptr_kind != NNMPC_HOST && ptr_kind != NNMPC_DEVICE)) {
    set_error("nnmpc_cstrs_flow: bad arguments (nb=%d)", nb);
    return NNMPC_EINVAL;
  }
  CstrsPar q;
  const int rc = cstrs_check(par, npar, sample_time, substeps, &q, "nnmpc_cstrs_flow");
  if (rc) return rc;
  if (nb == 0) return NNMPC_OK;
  GUARD_BEGIN
  if (int rc = check_device(__func__)) return rc;
  const size_t bx = (size_t)nb * 12 * 8, bu = (size_t)nb * 6 * 8, bp = (size_t)nb * 5 * 8;
  const double *xd = x, *ud = u, *pd = p;
  double* od = x_out;
  DevRes work;                                            // the staging of a host-pointer call: freed on every way out
  HIPCHK(hipGetDevice(&work.device));
  if (ptr_kind == NNMPC_HOST) {
    char* b = nullptr;
    if (int rc = work.alloc(&b, 2 * bx + bu + bp)) return rc;
    double *xh = (double*)b, *uh = (double*)(b + bx), *ph = (double*)(b + bx + bu);
    od = (double*)(b + bx + bu + bp);
    HIPCHK(hipMemcpy(xh, x, bx, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(uh, u, bu, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ph, p, bp, hipMemcpyHostToDevice));
    xd = xh; ud = uh; pd = ph;
  }
  hipLaunchKernelGGL(cstrs_flow_k, dim3((nb + CSTRS_THREADS - 1) / CSTRS_THREADS), dim3(CSTRS_THREADS), 0, 0, q, sample_time / substeps,
                     substeps, nb, xd, ud, pd, od);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  if (ptr_kind == NNMPC_HOST) HIPCHK(hipMemcpy(x_out, od, bx, hipMemcpyDeviceToHost));
  return NNMPC_OK;
  GUARD_END
}

}  // extern "C"
