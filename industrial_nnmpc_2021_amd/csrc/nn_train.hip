// Training step of the structured NN controller for gfx950 (f32 storage and accumulation, losses summed in fp64):
//   pred = us + MLP([x, (uprev), xs, us]) - MLP([xs, (us), xs, us]),  loss = mean (pred - u)^2,  Adam.
// Counterpart of train.py's torch step (RegulatorModel + torch.optim.Adam), reference cdu_train.py:40-62.
// One network per handle.  This file holds the kernels of a step, their enqueue order and the nnmpc_train_* entry points;
// the network's layout, padding, uploads, read-backs, dataset, events and argument checks are nn_train_host.h's, shared
// with the grouped trainer (nn_train_group.hip).
//
// A batch of B samples is stacked as the forward stacks it: pass 1 in rows [0, Bp), pass 2 in rows [Bp, 2Bp), Bp = B
// rounded up to 128, widths padded as nnmpc_nn_create pads them.  Per step:
//   gather      rows of the device-resident f32 dataset by index -> A_0                       (train_gather_k)
//   forward     A_l = relu(A_{l-1} W_l + b_l), every A_l kept; bias-free head                   (gemm_nt_f32_k)
//   output      pred, dZ_L = +-2 (pred - u) / (B nu) (zero on padding rows), fp64 loss partials  (train_output_k)
//   backward    dW_l = dZ_l' A_{l-1} as partial planes over row slices                          (gemm_tn_f32_k)
//               db_l partial column sums per 128 rows                                           (train_colsum_k)
//               dZ_{l-1} = (dZ_l W_l) * (A_{l-1} > 0) against the [in][out] copy of W_l          (gemm_nt_mask_k)
//   Adam        adds the planes in a fixed order, updates m, v, W and writes W in both layouts   (train_adam_w_k / _b_k)
// No atomics and no hand-off between workgroups of a launch: every sum has one fixed order, so a step is bit-identical
// from run to run.
//
// The unstructured forms (nnmpc_train_create_ex with NNMPC_NN_UNSTD / _UNSTD_RELU; reference cstrs_train_unstd.py:24-57):
//   pred = MLP([x, (uprev), xs, us]),  or relu of it.
// ONE pass, so a batch is M = Bp stacked rows (train_gather1_k); the head has a bias (and a ReLU) in its GEMM epilogue, a
// bias gradient (train_colsum_k over the head's dZ) and a bias Adam; the output kernel (train_output1_k) takes pred from the
// head as it is and, under the ReLU, zeroes dZ where pred <= 0.  Every other launch is the structured one at M rows.
//
// The tangent loss (nnmpc_train_create_tan, structured form; nn_train_dev.h has the arithmetic):
//   L = mean (pred - u)^2 + w mean (J d - t)^2,  J d the tangent of pred along the row's direction d = [dx, (duprev)].
// With w > 0 a batch is M = 3Bp stacked rows, the tangent rows in [2Bp, 3Bp), and the step keeps its 6 nlayers launches:
// every one below is a variant of the plain launch in the same place.
//   gather      all three blocks                                                                 (train_gather_tan_k)
//   forward     hidden layers: a pass-1 row tile and its tangent tile in one workgroup, pass 2    (gemm_nt_f32_pair_k)
//               as before; the head is bias-free and linear: the plain launch over 3Bp rows      (gemm_nt_f32_k)
//   output      the plain output and dZ'_L = 2 w (J d - t) / (B nu), a second set of partials     (train_output_tan_k)
//   backward    dW over 3Bp rows; db over the first 2Bp (tangent rows carry no bias gradient);    (gemm_tn_f32_k, train_colsum_k)
//               dA over 3Bp rows, the mask row of a tangent row being its pass-1 row              (gemm_nt_mask_wrap_k)
// With w == 0 the handle runs the plain step, launch for launch.
//
// nnmpc_train_create_tan_ex: D directions per row and, whole_input, directions over [dx, (duprev), dxs, dus].  The D tangent
// blocks of pass 1 follow the two primal blocks and, whole input, D of pass 2 follow those: M = (2 + D) Bp or (2 + 2D) Bp.
// Still 6 nlayers launches: the gather and the output kernel take D and the form, the hidden forward is a fan -- a primal
// row tile and its D tangent tiles in one workgroup (gemm_nt_f32_fan_k; whole input: the pass-2 tiles are fans too) --, and
// the mask of a row tile in block k >= 2 is the same tile of block (k - 2) / D.  D = 1 in [dx, (duprev)] launches the pair.
#include "gemm_kernels.h"
#include "tile_gemm_tn.h"
#include "nn_train_host.h"

using namespace nnmpc;

namespace {

// The kernels below are one workgroup function of nn_train_dev.h each, at this launch's block coordinates.
__global__ __launch_bounds__(128) void train_gather_k(float* __restrict__ in, int ldk, int Bp, int B, int nx, int nu,
                                                      int with_uprev, const float* __restrict__ x,
                                                      const float* __restrict__ uprev, const float* __restrict__ xs,
                                                      const float* __restrict__ us, const int* __restrict__ idx, int first) {
  train_gather_rows(in, ldk, Bp, B, nx, nu, with_uprev, x, uprev, xs, us, idx, first, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(256) void train_output_k(float* __restrict__ dz, const float* __restrict__ o, int ldo, int Bp,
                                                      int B, int nu, const float* __restrict__ us,
                                                      const float* __restrict__ u, const int* __restrict__ idx, int first,
                                                      float gscale, double* __restrict__ partial) {
  train_output_block(dz, o, ldo, Bp, B, nu, us, u, idx, first, gscale, partial, blockIdx.x);
}

// The unstructured forms: one row per sample, the head's output is the prediction.
__global__ __launch_bounds__(128) void train_gather1_k(float* __restrict__ in, int ldk, int Bp, int B, int nx, int nu,
                                                       int with_uprev, const float* __restrict__ x,
                                                       const float* __restrict__ uprev, const float* __restrict__ xs,
                                                       const float* __restrict__ us, const int* __restrict__ idx, int first) {
  train_gather_rows1(in, ldk, Bp, B, nx, nu, with_uprev, x, uprev, xs, us, idx, first, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(256) void train_output1_k(float* __restrict__ dz, const float* __restrict__ o, int ldo, int B,
                                                       int nu, int head_relu, const float* __restrict__ u,
                                                       const int* __restrict__ idx, int first, float gscale,
                                                       double* __restrict__ partial) {
  train_output1_block(dz, o, ldo, B, nu, head_relu, u, idx, first, gscale, partial, blockIdx.x);
}

// The tangent loss: every row block; the plain output plus the tangent rows; both sums.
__global__ __launch_bounds__(128) void train_gather_tan_k(float* __restrict__ in, int ldk, int Bp, int B, int nx, int nu,
                                                          int with_uprev, int D, int whole, const float* __restrict__ x,
                                                          const float* __restrict__ uprev, const float* __restrict__ xs,
                                                          const float* __restrict__ us, const float* __restrict__ tdx,
                                                          const float* __restrict__ tdup, const float* __restrict__ tdxs,
                                                          const float* __restrict__ tdus, const int* __restrict__ idx, int first) {
  train_gather_rows(in, ldk, Bp, B, nx, nu, with_uprev, x, uprev, xs, us, idx, first, blockIdx.x, gridDim.x);
  train_gather_tan_rows(in, ldk, Bp, B, nx, nu, with_uprev, D, whole, tdx, tdup, tdxs, tdus, idx, first, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(256) void train_output_tan_k(float* __restrict__ dz, const float* __restrict__ o, int ldo, int Bp,
                                                          int B, int nu, int D, int whole, const float* __restrict__ us,
                                                          const float* __restrict__ u, const float* __restrict__ t,
                                                          const float* __restrict__ tdus, const int* __restrict__ idx, int first,
                                                          float gscale, float gw, double* __restrict__ partial,
                                                          double* __restrict__ partial_tan) {
  train_output_tan_block(dz, o, ldo, Bp, B, nu, D, whole, us, u, t, tdus, idx, first, gscale, gw, partial, partial_tan, blockIdx.x);
}

__global__ void train_loss_finish_tan_k(const double* __restrict__ partial, const double* __restrict__ partial_tan, int np,
                                        double scale, double scale_tan, double weight, double w, double* __restrict__ loss,
                                        double* __restrict__ acc) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  train_loss_finish_tan(partial, partial_tan, np, scale, scale_tan, weight, w, loss, acc);
}

// Hidden-layer forward under the tangent loss.  Grid (N/NB, 2Bp/NB): the low blockIdx.y are the pass-1 row tiles, each with
// its tangent tile (twice the work: they start first); the others are pass 2, the plain tile.
template <int NB>
__global__ __launch_bounds__(256) void gemm_nt_f32_pair_k(float* __restrict__ C, size_t ldc, const float* __restrict__ A,
                                                          size_t lda, const float* __restrict__ B, size_t ldb, int K,
                                                          const float* __restrict__ bias, int Bp) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if ((int)blockIdx.y < Bp / NB) train_fwd_pair_tile<NB>(C, ldc, A, lda, B, ldb, K, bias, Bp, blockIdx.y, blockIdx.x, lds);
  else train_fwd_tile<NB, true, true>(C, ldc, A, lda, B, ldb, K, bias, blockIdx.y, blockIdx.x, lds);
}

// The same with D directions per row.  Same grid: a pass-1 row tile is a fan of 1 + D tiles, its tangents from row 2 Bp on; a
// pass-2 row tile is the plain tile, or (whole input) a fan whose tangents start D blocks further down, at (2 + D) Bp.
template <int NB>
__global__ __launch_bounds__(256) void gemm_nt_f32_fan_k(float* __restrict__ C, size_t ldc, const float* __restrict__ A,
                                                         size_t lda, const float* __restrict__ B, size_t ldb, int K,
                                                         const float* __restrict__ bias, int Bp, int D, int whole) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if ((int)blockIdx.y < Bp / NB) train_fwd_fan_tile<NB>(C, ldc, A, lda, B, ldb, K, bias, Bp, D, 2 * Bp, blockIdx.y, blockIdx.x, lds);
  else if (whole) train_fwd_fan_tile<NB>(C, ldc, A, lda, B, ldb, K, bias, Bp, D, (1 + D) * Bp, blockIdx.y, blockIdx.x, lds);
  else train_fwd_tile<NB, true, true>(C, ldc, A, lda, B, ldb, K, bias, blockIdx.y, blockIdx.x, lds);
}

__global__ void train_loss_finish_k(const double* __restrict__ partial, int np, double scale, double w,
                                    double* __restrict__ loss, double* __restrict__ acc) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  train_loss_finish(partial, np, scale, w, loss, acc);
}

// Grid (N/NB, M/NB, slices).
template <int NB>
__global__ __launch_bounds__(256) void gemm_tn_f32_k(float* __restrict__ P, size_t plane, size_t ldp,
                                                     const float* __restrict__ A, size_t lda,
                                                     const float* __restrict__ B, size_t ldb, int rows, int slice_rows) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  train_tn_tile<NB>(P, plane, ldp, A, lda, B, ldb, rows, slice_rows, blockIdx.x, blockIdx.y, blockIdx.z, lds);
}

template <int NB>
__global__ __launch_bounds__(256) void gemm_nt_mask_k(float* __restrict__ C, size_t ldc, const float* __restrict__ A,
                                                      size_t lda, const float* __restrict__ B, size_t ldb, int K,
                                                      const float* __restrict__ act) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  train_nt_mask_tile<NB>(C, ldc, A, lda, B, ldb, K, act, blockIdx.x, blockIdx.y, lds);
}

// gemm_nt_mask_k over the stacked rows of the tangent loss: a row tile in block k >= 2 (blocks of Bp rows) takes its mask from
// the same tile of block (k - 2) / D, the primal rows its tangents belong to: pass 1 for the first D tangent blocks, pass 2
// for the D behind them (tiles never straddle blocks: Bp is a multiple of 128).
template <int NB>
__global__ __launch_bounds__(256) void gemm_nt_mask_wrap_k(float* __restrict__ C, size_t ldc, const float* __restrict__ A,
                                                           size_t lda, const float* __restrict__ B, size_t ldb, int K,
                                                           const float* __restrict__ act, int Bp, int D) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int k = (int)blockIdx.y * NB / Bp;
  const float* mask = k >= 2 ? act - (size_t)(k - (k - 2) / D) * Bp * ldc : act;
  train_nt_mask_tile<NB>(C, ldc, A, lda, B, ldb, K, mask, blockIdx.x, blockIdx.y, lds);
}

// Grid (N/64, rows/128).
__global__ __launch_bounds__(256) void train_colsum_k(float* __restrict__ P, const float* __restrict__ dz, int ld) {
  train_colsum_block(P, dz, ld, blockIdx.x, blockIdx.y);
}

__global__ void train_plane_sum_k(float* __restrict__ g, const float* __restrict__ P, size_t plane, int S) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < plane) g[i] = plane_sum(P, plane, S, i);
}

// Grid (kpad/64, npad/64).
__global__ __launch_bounds__(256) void train_adam_w_k(float* __restrict__ Wt, float* __restrict__ Wk, float* __restrict__ m,
                                                      float* __restrict__ v, const float* __restrict__ P, size_t plane, int S,
                                                      int kpad, int npad, AdamCoef k) {
  train_adam_w_tile(Wt, Wk, m, v, P, plane, S, kpad, npad, k, blockIdx.x, blockIdx.y);
}

__global__ void train_adam_b_k(float* __restrict__ b, float* __restrict__ m, float* __restrict__ v,
                               const float* __restrict__ P, int npad, int S, AdamCoef k) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < npad) b[i] = adam_entry(plane_sum(P, (size_t)npad, S, (size_t)i), m + i, v + i, b[i], k);
}

}  // namespace

struct nnmpc_train {
  TrainCommon c;
  Member m;
  std::vector<int> slices;                                  // of the last backward pass, per layer
  char* arena = nullptr;                                    // the network's buffers, its acc word, then grad
  float* grad = nullptr;                                    // summed gradient (nnmpc_train_grad only): per layer gW [N][K] then gb [N]
  // What nnmpc_train_last_losses reads: the loss words of a batch (LAST_BATCH) or the running sums over last_den (LAST_SUMS);
  // last_tan: that call ran the tangent step, so the words hold L, mse, tan_mse (otherwise L alone, which is the mse).
  enum { LAST_NONE, LAST_BATCH, LAST_SUMS } last = LAST_NONE;
  bool last_tan = false;
  double last_den = 1.0;
};

namespace {

template <int NB>
void launch_fwd_pair(hipStream_t s, float* C, size_t ldc, const float* A, size_t lda, const float* Wt, size_t ldb, int Bp, int N,
                     int K, const float* bias) {
  hipLaunchKernelGGL((gemm_nt_f32_pair_k<NB>), dim3(N / NB, 2 * Bp / NB), dim3(256), TileCfg<NB>::LDS_FLOATS * 4, s,
                     C, ldc, A, lda, Wt, ldb, K, bias, Bp);
}

template <int NB>
void launch_fwd_fan(hipStream_t s, float* C, size_t ldc, const float* A, size_t lda, const float* Wt, size_t ldb, int Bp, int N,
                    int K, const float* bias, int D, int whole) {
  hipLaunchKernelGGL((gemm_nt_f32_fan_k<NB>), dim3(N / NB, 2 * Bp / NB), dim3(256), TileCfg<NB>::LDS_FLOATS * 4, s,
                     C, ldc, A, lda, Wt, ldb, K, bias, Bp, D, whole);
}

template <int NB, bool RELU, bool BIAS>
void launch_fwd(hipStream_t s, float* C, size_t ldc, const float* A, size_t lda, const float* Wt, size_t ldb, int M, int N,
                int K, const float* bias) {
  hipLaunchKernelGGL((gemm_nt_f32_k<NB, RELU, BIAS>), dim3(N / NB, M / NB), dim3(256), TileCfg<NB>::LDS_FLOATS * 4, s,
                     C, ldc, A, lda, Wt, ldb, K, bias);
}

// Gather, forward, output kernel and (backward) the gradient planes of one batch on the handle's stream; no host wait.
// idx: device row list (nullptr: rows first .. first + B - 1).  The loss goes to the network's loss word = loss_scale * sum
// of squares, and acc += acc_w * that.  With the tangent term in the loss (tan_active) every launch is its tangent variant
// over M = (2 + D) Bp (whole input: (2 + 2D) Bp) rows, the loss words are L, mse, tan_mse and acc[0..2] take all three.
int enqueue_batch(nnmpc_train* h, int B, const int* idx, int first, bool backward, double loss_scale, double acc_w, size_t set) {
  TrainCommon& c = h->c;
  const GMember& mem = h->m.mem;
  hipStream_t s = c.stream;
  const bool tan = tan_active(c);
  const int D = c.tan_dirs, whole = c.tan_whole;
  const bool fan = D != 1 || whole;                        // D = 1 in [dx, (duprev)] keeps the pair launch
  const int L = c.L, Bp = pad128_host(B), M = train_rows_tan(c.form, Bp, tan, D, whole);
  const bool un = c.form != NNMPC_NN_STRUCTURED, hrelu = c.form == NNMPC_NN_UNSTD_RELU;
  EvSet e;
  if (int rc = ev_set(c, set, &e)) return rc;
  if (tan)
    hipLaunchKernelGGL(train_gather_tan_k, dim3(std::min(Bp, 2048)), dim3(128), 0, s, h->m.lay[0].ain, h->m.lay[0].K, Bp, B, c.nx, c.nu,
                       c.with_uprev, D, whole, c.dx, c.dup, c.dxs, c.dus, c.tdx, c.tdup, c.tdxs, c.tdus, idx, first);
  else if (un)
    hipLaunchKernelGGL(train_gather1_k, dim3(std::min(Bp, 2048)), dim3(128), 0, s, h->m.lay[0].ain, h->m.lay[0].K, Bp, B, c.nx, c.nu,
                       c.with_uprev, c.dx, c.dup, c.dxs, c.dus, idx, first);
  else
    hipLaunchKernelGGL(train_gather_k, dim3(std::min(Bp, 2048)), dim3(128), 0, s, h->m.lay[0].ain, h->m.lay[0].K, Bp, B, c.nx, c.nu,
                       c.with_uprev, c.dx, c.dup, c.dxs, c.dus, idx, first);
  hipEventRecord(e.f0, s);
  for (int l = 0; l < L; ++l) {
    const GLayer& d = h->m.lay[l];
    const int K = d.K, N = d.N;
    const bool last = l == L - 1;
    if (tan && !last && fan) {
      if (N % 128 == 0) launch_fwd_fan<128>(s, d.aout, N, d.ain, K, d.Wt, K, Bp, N, K, d.b, D, whole);
      else launch_fwd_fan<64>(s, d.aout, N, d.ain, K, d.Wt, K, Bp, N, K, d.b, D, whole);
    } else if (tan && !last) {
      if (N % 128 == 0) launch_fwd_pair<128>(s, d.aout, N, d.ain, K, d.Wt, K, Bp, N, K, d.b);
      else launch_fwd_pair<64>(s, d.aout, N, d.ain, K, d.Wt, K, Bp, N, K, d.b);
    } else if (N % 128 == 0) {
      if (last && hrelu) launch_fwd<128, true, true>(s, d.aout, N, d.ain, K, d.Wt, K, M, N, K, d.b);
      else if (last && un) launch_fwd<128, false, true>(s, d.aout, N, d.ain, K, d.Wt, K, M, N, K, d.b);
      else if (last) launch_fwd<128, false, false>(s, d.aout, N, d.ain, K, d.Wt, K, M, N, K, nullptr);
      else launch_fwd<128, true, true>(s, d.aout, N, d.ain, K, d.Wt, K, M, N, K, d.b);
    } else {
      if (last && hrelu) launch_fwd<64, true, true>(s, d.aout, N, d.ain, K, d.Wt, K, M, N, K, d.b);
      else if (last && un) launch_fwd<64, false, true>(s, d.aout, N, d.ain, K, d.Wt, K, M, N, K, d.b);
      else if (last) launch_fwd<64, false, false>(s, d.aout, N, d.ain, K, d.Wt, K, M, N, K, nullptr);
      else launch_fwd<64, true, true>(s, d.aout, N, d.ain, K, d.Wt, K, M, N, K, d.b);
    }
  }
  hipEventRecord(e.f1, s);
  const GLayer& head = h->m.lay[L - 1];
  const double gs = 2.0 / ((double)B * c.nu);
  double* partial_tan = mem.partial + c.cap_batch / 64;
  if (tan)
    hipLaunchKernelGGL(train_output_tan_k, dim3(Bp / 64), dim3(256), 0, s, backward ? mem.dz[0] : nullptr, head.aout, head.N, Bp, B,
                       c.nu, D, whole, c.dus, c.du, c.tt, c.tdus, idx, first, (float)gs, (float)(gs / D * c.tan_w), mem.partial, partial_tan);
  else if (un)
    hipLaunchKernelGGL(train_output1_k, dim3(Bp / 64), dim3(256), 0, s, backward ? mem.dz[0] : nullptr, head.aout, head.N, B,
                       c.nu, hrelu ? 1 : 0, c.du, idx, first, (float)gs, mem.partial);
  else
    hipLaunchKernelGGL(train_output_k, dim3(Bp / 64), dim3(256), 0, s, backward ? mem.dz[0] : nullptr, head.aout, head.N, Bp, B,
                       c.nu, c.dus, c.du, idx, first, (float)gs, mem.partial);
  if (tan)
    hipLaunchKernelGGL(train_loss_finish_tan_k, dim3(1), dim3(64), 0, s, mem.partial, partial_tan, Bp / 64, loss_scale, loss_scale / D, acc_w, c.tan_w,
                       mem.loss, mem.acc);
  else
    hipLaunchKernelGGL(train_loss_finish_k, dim3(1), dim3(64), 0, s, mem.partial, Bp / 64, loss_scale, acc_w, mem.loss, mem.acc);
  hipEventRecord(e.b0, s);
  if (backward) {
    int cur = 0;
    for (int l = L - 1; l >= 0; --l) {
      const GLayer& d = h->m.lay[l];
      const int K = d.K, N = d.N;
      const float* dZ = mem.dz[cur];
      const bool big = N % 128 == 0 && K % 128 == 0;
      int slice_rows = 0;
      const int S = member_slices(c, h->m, l, M, &slice_rows);
      if (S > h->m.max_slices[l]) { set_error("nnmpc_train: %d dW slices for layer %d, planes for %d", S, l, h->m.max_slices[l]); return NNMPC_EINVAL; }
      h->slices[l] = S;
      const size_t plane = (size_t)N * K;
      if (big)
        hipLaunchKernelGGL(gemm_tn_f32_k<128>, dim3(K / 128, N / 128, S), dim3(256), TileCfgTN<128>::LDS_FLOATS * 4, s,
                           d.planes, plane, (size_t)K, dZ, (size_t)N, d.ain, (size_t)K, M, slice_rows);
      else
        hipLaunchKernelGGL(gemm_tn_f32_k<64>, dim3(K / 64, N / 64, S), dim3(256), TileCfgTN<64>::LDS_FLOATS * 4, s,
                           d.planes, plane, (size_t)K, dZ, (size_t)N, d.ain, (size_t)K, M, slice_rows);
      if (has_bias(c.form, L, l))
        hipLaunchKernelGGL(train_colsum_k, dim3(N / 64, train_rows(c.form, Bp) / 128), dim3(256), 0, s, d.bplanes, dZ, N);   // never the tangent rows
      if (l > 0 && tan) {                                    // the same over M rows, a tangent row masked by the primal row it belongs to
        if (K % 128 == 0)
          hipLaunchKernelGGL(gemm_nt_mask_wrap_k<128>, dim3(K / 128, M / 128), dim3(256), TileCfg<128>::LDS_FLOATS * 4, s,
                             mem.dz[cur ^ 1], (size_t)K, dZ, (size_t)N, d.Wk, (size_t)N, N, d.ain, Bp, D);
        else
          hipLaunchKernelGGL(gemm_nt_mask_wrap_k<64>, dim3(K / 64, M / 64), dim3(256), TileCfg<64>::LDS_FLOATS * 4, s,
                             mem.dz[cur ^ 1], (size_t)K, dZ, (size_t)N, d.Wk, (size_t)N, N, d.ain, Bp, D);
        cur ^= 1;
      } else if (l > 0) {                                    // dZ_{l-1} [M][K] = (dZ_l [M][N] Wk_l [K][N]') * mask(A_l input = ain)
        if (K % 128 == 0)
          hipLaunchKernelGGL(gemm_nt_mask_k<128>, dim3(K / 128, M / 128), dim3(256), TileCfg<128>::LDS_FLOATS * 4, s,
                             mem.dz[cur ^ 1], (size_t)K, dZ, (size_t)N, d.Wk, (size_t)N, N, d.ain);
        else
          hipLaunchKernelGGL(gemm_nt_mask_k<64>, dim3(K / 64, M / 64), dim3(256), TileCfg<64>::LDS_FLOATS * 4, s,
                             mem.dz[cur ^ 1], (size_t)K, dZ, (size_t)N, d.Wk, (size_t)N, N, d.ain);
        cur ^= 1;
      }
    }
  }
  hipEventRecord(e.b1, s);
  return NNMPC_OK;
}

// The Adam update of every tensor from the planes of the last backward pass of a batch of Bp padded rows.
void enqueue_adam(nnmpc_train* h, int Bp) {
  const TrainCommon& c = h->c;
  ++h->m.t;
  const AdamCoef k = adam_coef(c.lr, c.beta1, c.beta2, c.eps, h->m.t);
  for (int l = 0; l < c.L; ++l) {
    const GLayer& d = h->m.lay[l];
    hipLaunchKernelGGL(train_adam_w_k, dim3(d.K / 64, d.N / 64), dim3(256), 0, c.stream, d.Wt, d.Wk, d.mW, d.vW,
                       d.planes, (size_t)d.N * d.K, h->slices[l], d.K, d.N, k);
    if (has_bias(c.form, c.L, l))
      hipLaunchKernelGGL(train_adam_b_k, dim3((d.N + 255) / 256), dim3(256), 0, c.stream, d.b, d.mb, d.vb, d.bplanes, d.N, train_rows(c.form, Bp) / 128, k);
  }
}

// Checks a batch of the caller's rows, uploads it and enqueues its forward and backward pass; the loss is the batch's own.
int enqueue_rows(nnmpc_train* h, const char* who, int32_t B, const int32_t* rows) {
  TrainCommon& c = h->c;
  if (int rc = check_batch(c, who, B)) return rc;
  if (int rc = check_rows(c, who, (size_t)B, rows)) return rc;
  if (int rc = check_tangents(c, who)) return rc;
  HIPCHK(hipSetDevice(c.device));
  if (int rc = staged_upload(c, nullptr, 0, rows, (size_t)B)) return rc;
  hipEventRecord(c.e0, c.stream);
  if (int rc = enqueue_batch(h, B, (const int*)c.dcall, 0, true, 1.0 / ((double)B * c.nu), 0.0, 0)) return rc;
  c.nsets = 1;
  h->last = nnmpc_train::LAST_BATCH; h->last_tan = tan_active(c); h->last_den = 1.0;
  return NNMPC_OK;
}
}  // namespace

extern "C" {

int nnmpc_train_destroy(nnmpc_train* h) {
  if (!h) return NNMPC_OK;
  h->c.res.release();
  delete h;
  return NNMPC_OK;
}

// The create entry points; `who` is the one that was called.  tan: a tangent handle (nnmpc_train_create_tan).
static int train_create(const char* who, nnmpc_train** out, int32_t nlayers, const int32_t* dims, const double* const* W,
                        const double* const* b, int32_t nx, int32_t nu, int32_t with_uprev, int32_t max_batch,
                        double lr, double beta1, double beta2, double eps, int32_t form, bool tan = false, int32_t dirs = 1,
                        int32_t whole_input = 0) {
  GUARD_BEGIN
  if (!out || nlayers < 1 || !dims || !W || !b || nx <= 0 || nu <= 0 || max_batch < 1) { set_error("%s: bad arguments", who); return NNMPC_EINVAL; }
  if (int rc = check_form(who, form)) return rc;
  if (dirs < 1 || dirs > NNMPC_TAN_MAX_DIRS) { set_error("%s: %d directions per row (1 .. NNMPC_TAN_MAX_DIRS = %d)", who, dirs, NNMPC_TAN_MAX_DIRS); return NNMPC_EINVAL; }
  if (whole_input != 0 && whole_input != 1) { set_error("%s: whole_input %d (0 or 1)", who, whole_input); return NNMPC_EINVAL; }
  if (tan && form != NNMPC_NN_STRUCTURED) { set_error("%s: form %d: the tangent loss is built for the structured form only (NNMPC_NN_STRUCTURED)", who, form); return NNMPC_EINVAL; }
  if (int rc = check_network(who, "", nlayers, dims, W, b, nx, nu, with_uprev, form)) return rc;
  if (int rc = check_adam(who, lr, beta1, beta2, eps)) return rc;
  if (int rc = check_device(who)) return rc;
  Building<nnmpc_train, nnmpc_train_destroy> guard(new nnmpc_train());   // released into *out at the end; destroyed on any other way out
  nnmpc_train* h = guard.get();
  TrainCommon& c = h->c;
  if (int rc = common_init(who, c, nlayers, nx, nu, with_uprev, max_batch, lr, beta1, beta2, eps, form)) return rc;
  c.tan = tan ? 1 : 0; c.tan_dirs = dirs; c.tan_whole = whole_input;   // before the shapes: workspaces, planes and slices for (2 + D) or (2 + 2D) cap_batch rows
  HIPCHK(hipFuncSetAttribute((const void*)gemm_nt_f32_k<128, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, TileCfg<128>::LDS_FLOATS * 4));
  HIPCHK(hipFuncSetAttribute((const void*)gemm_nt_f32_k<128, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, TileCfg<128>::LDS_FLOATS * 4));
  HIPCHK(hipFuncSetAttribute((const void*)gemm_nt_f32_k<128, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, TileCfg<128>::LDS_FLOATS * 4));   // the unstructured head
  HIPCHK(hipFuncSetAttribute((const void*)gemm_nt_mask_k<128>, hipFuncAttributeMaxDynamicSharedMemorySize, TileCfg<128>::LDS_FLOATS * 4));
  if (tan) {
    HIPCHK(hipFuncSetAttribute((const void*)gemm_nt_f32_pair_k<128>, hipFuncAttributeMaxDynamicSharedMemorySize, TileCfg<128>::LDS_FLOATS * 4));
    HIPCHK(hipFuncSetAttribute((const void*)gemm_nt_f32_fan_k<128>, hipFuncAttributeMaxDynamicSharedMemorySize, TileCfg<128>::LDS_FLOATS * 4));
    HIPCHK(hipFuncSetAttribute((const void*)gemm_nt_mask_wrap_k<128>, hipFuncAttributeMaxDynamicSharedMemorySize, TileCfg<128>::LDS_FLOATS * 4));
  }
  HIPCHK(hipFuncSetAttribute((const void*)gemm_tn_f32_k<128>, hipFuncAttributeMaxDynamicSharedMemorySize, TileCfgTN<128>::LDS_FLOATS * 4));
  member_shapes(c, h->m, dims);
  h->slices.assign(nlayers, 1);
  size_t grad_floats = 0;
  for (int l = 0; l < nlayers; ++l) grad_floats += (size_t)h->m.npad[l] * (h->m.kpad[l] + 1);
  const size_t acc_at = layout_member(c, h->m, nullptr, 0), grad_at = acc_at + 4096, bytes = grad_at + grad_floats * 4;
  if (int rc = c.res.alloc(&h->arena, bytes)) return rc;
  layout_member(c, h->m, h->arena, 0);
  h->m.mem.acc = (double*)(h->arena + acc_at);
  h->grad = (float*)(h->arena + grad_at);
  if (int rc = upload_member(c, h->m, W, b)) return rc;
  *out = guard.release();
  return NNMPC_OK;
  GUARD_END
}

int nnmpc_train_create(nnmpc_train** out, int32_t nlayers, const int32_t* dims, const double* const* W,
                       const double* const* b, int32_t nx, int32_t nu, int32_t with_uprev, int32_t max_batch,
                       double lr, double beta1, double beta2, double eps) {
  return train_create(__func__, out, nlayers, dims, W, b, nx, nu, with_uprev, max_batch, lr, beta1, beta2, eps, NNMPC_NN_STRUCTURED);
}

int nnmpc_train_create_ex(nnmpc_train** out, int32_t nlayers, const int32_t* dims, const double* const* W,
                          const double* const* b, int32_t nx, int32_t nu, int32_t with_uprev, int32_t max_batch,
                          double lr, double beta1, double beta2, double eps, int32_t form) {
  return train_create(__func__, out, nlayers, dims, W, b, nx, nu, with_uprev, max_batch, lr, beta1, beta2, eps, form);
}

int nnmpc_train_create_tan(nnmpc_train** out, int32_t nlayers, const int32_t* dims, const double* const* W,
                           const double* const* b, int32_t nx, int32_t nu, int32_t with_uprev, int32_t max_batch,
                           double lr, double beta1, double beta2, double eps, int32_t form) {
  return train_create(__func__, out, nlayers, dims, W, b, nx, nu, with_uprev, max_batch, lr, beta1, beta2, eps, form, true);
}

int nnmpc_train_create_tan_ex(nnmpc_train** out, int32_t nlayers, const int32_t* dims, const double* const* W,
                              const double* const* b, int32_t nx, int32_t nu, int32_t with_uprev, int32_t max_batch,
                              double lr, double beta1, double beta2, double eps, int32_t form, int32_t dirs, int32_t whole_input) {
  return train_create(__func__, out, nlayers, dims, W, b, nx, nu, with_uprev, max_batch, lr, beta1, beta2, eps, form, true, dirs, whole_input);
}

int nnmpc_train_set_tangents(nnmpc_train* h, int32_t n, const double* dx, const double* duprev, const double* t, int32_t ptr_kind) {
  GUARD_BEGIN
  if (!h) { set_error("nnmpc_train_set_tangents: bad arguments"); return NNMPC_EINVAL; }
  if (h->c.tan && (h->c.tan_dirs != 1 || h->c.tan_whole)) { set_error("nnmpc_train_set_tangents: the handle has %d directions per row%s: nnmpc_train_set_tangents_ex takes them", h->c.tan_dirs, h->c.tan_whole ? " over the whole input" : ""); return NNMPC_EINVAL; }
  return set_tangents(__func__, h->c, n, 1, dx, duprev, nullptr, nullptr, t, ptr_kind);
  GUARD_END
}

int nnmpc_train_set_tangents_ex(nnmpc_train* h, int32_t n, int32_t dirs, const double* dx, const double* duprev, const double* dxs,
                                const double* dus, const double* t, int32_t ptr_kind) {
  GUARD_BEGIN
  if (!h) { set_error("nnmpc_train_set_tangents_ex: bad arguments"); return NNMPC_EINVAL; }
  return set_tangents(__func__, h->c, n, dirs, dx, duprev, dxs, dus, t, ptr_kind);
  GUARD_END
}

int nnmpc_train_set_tan_weight(nnmpc_train* h, double w) {
  if (!h) { set_error("nnmpc_train_set_tan_weight: bad arguments"); return NNMPC_EINVAL; }
  if (!h->c.tan) { set_error("nnmpc_train_set_tan_weight: a plain handle has no tangent loss (nnmpc_train_create_tan builds the handle that has)"); return NNMPC_EINVAL; }
  if (!(w >= 0.0) || !isfinite(w)) { set_error("nnmpc_train_set_tan_weight: weight %g (finite and >= 0)", w); return NNMPC_EINVAL; }
  h->c.tan_w = w;
  return NNMPC_OK;
}

int nnmpc_train_last_losses(nnmpc_train* h, double* mse, double* tan_mse) {
  GUARD_BEGIN
  if (!h) { set_error("nnmpc_train_last_losses: bad arguments"); return NNMPC_EINVAL; }
  if (h->last == nnmpc_train::LAST_NONE) { set_error("nnmpc_train_last_losses: no grad, step, epoch or eval yet"); return NNMPC_EINVAL; }
  HIPCHK(hipSetDevice(h->c.device));
  double v[3] = {0.0, 0.0, 0.0};
  if (int rc = read_doubles(h->c, h->last == nnmpc_train::LAST_BATCH ? h->m.mem.loss : h->m.mem.acc, v, h->last_tan ? 3 : 1)) return rc;
  if (mse) *mse = (h->last_tan ? v[1] : v[0]) / h->last_den;   // without the tangent term the loss is the mse
  if (tan_mse) *tan_mse = h->last_tan ? v[2] / h->last_den : 0.0;
  return NNMPC_OK;
  GUARD_END
}

int nnmpc_train_set_data(nnmpc_train* h, int32_t n, const double* x, const double* uprev, const double* xs, const double* us,
                         const double* u, int32_t ptr_kind) {
  GUARD_BEGIN
  if (!h) { set_error("nnmpc_train_set_data: bad arguments"); return NNMPC_EINVAL; }
  return set_data(__func__, h->c, n, x, uprev, xs, us, u, ptr_kind);
  GUARD_END
}

int nnmpc_train_grad(nnmpc_train* h, int32_t B, const int32_t* rows, double* loss, double* const* gW, double* const* gb) {
  GUARD_BEGIN
  if (!h || !rows) { set_error("nnmpc_train_grad: bad arguments"); return NNMPC_EINVAL; }
  if (int rc = enqueue_rows(h, __func__, B, rows)) return rc;
  TrainCommon& c = h->c;
  float* at = h->grad;                                      // the planes added by the one plane_sum() the Adam kernels use
  for (int l = 0; l < c.L; ++l) {
    const GLayer& d = h->m.lay[l];
    const size_t plane = (size_t)d.N * d.K;
    hipLaunchKernelGGL(train_plane_sum_k, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, c.stream, at, d.planes, plane, h->slices[l]);
    if (has_bias(c.form, c.L, l))
      hipLaunchKernelGGL(train_plane_sum_k, dim3((d.N + 255) / 256), dim3(256), 0, c.stream, at + plane, d.bplanes, (size_t)d.N, train_rows(c.form, pad128_host(B)) / 128);
    at += plane + d.N;
  }
  hipEventRecord(c.e1, c.stream);
  double lv = 0.0;
  if (int rc = read_doubles(c, h->m.mem.loss, &lv, 1)) return rc;
  if (loss) *loss = lv;
  return read_back(c, h->m, h->grad, gW, gb);
  GUARD_END
}

int nnmpc_train_step(nnmpc_train* h, int32_t B, const int32_t* rows, double* loss) {
  GUARD_BEGIN
  if (!h || !rows) { set_error("nnmpc_train_step: bad arguments"); return NNMPC_EINVAL; }
  if (int rc = enqueue_rows(h, __func__, B, rows)) return rc;
  enqueue_adam(h, pad128_host(B));
  hipEventRecord(h->c.e1, h->c.stream);
  if (loss) return read_doubles(h->c, h->m.mem.loss, loss, 1);
  return NNMPC_OK;
  GUARD_END
}

int nnmpc_train_epoch(nnmpc_train* h, int32_t nrows, const int32_t* perm, int32_t batch, double* loss) {
  GUARD_BEGIN
  if (!h || !perm || nrows < 1) { set_error("nnmpc_train_epoch: bad arguments"); return NNMPC_EINVAL; }
  TrainCommon& c = h->c;
  if (int rc = check_batch(c, __func__, batch)) return rc;
  if (int rc = check_rows(c, __func__, (size_t)nrows, perm)) return rc;
  if (int rc = check_tangents(c, __func__)) return rc;
  HIPCHK(hipSetDevice(c.device));
  hipStream_t s = c.stream;
  if (int rc = staged_upload(c, nullptr, 0, perm, (size_t)nrows)) return rc;
  HIPCHK(hipMemsetAsync(h->m.mem.acc, 0, 24, s));           // L, and under the tangent loss mse and tan_mse
  hipEventRecord(c.e0, s);
  size_t set = 0;
  for (int i = 0; i < nrows; i += batch, ++set) {
    const int B = std::min(batch, nrows - i);              // the last batch is the short one
    if (int rc = enqueue_batch(h, B, (const int*)c.dcall + i, 0, true, 1.0 / ((double)B * c.nu), (double)B, set)) return rc;
    enqueue_adam(h, pad128_host(B));
  }
  c.nsets = set;
  h->last = nnmpc_train::LAST_SUMS; h->last_tan = tan_active(c); h->last_den = (double)nrows;
  hipEventRecord(c.e1, s);
  double sum = 0.0;
  if (int rc = read_doubles(c, h->m.mem.acc, &sum, 1)) return rc;
  if (loss) *loss = sum / (double)nrows;
  return NNMPC_OK;
  GUARD_END
}

int nnmpc_train_eval(nnmpc_train* h, int32_t first, int32_t count, double* mse) {
  GUARD_BEGIN
  if (!h || !mse) { set_error("nnmpc_train_eval: bad arguments"); return NNMPC_EINVAL; }
  TrainCommon& c = h->c;
  if (int rc = check_data(c, __func__)) return rc;
  if (first < 0 || count < 1 || (int64_t)first + count > c.n) { set_error("nnmpc_train_eval: rows [%d, %d + %d) outside [0, %d)", first, first, count, c.n); return NNMPC_EINVAL; }
  if (int rc = check_tangents(c, __func__)) return rc;
  HIPCHK(hipSetDevice(c.device));
  hipStream_t s = c.stream;
  HIPCHK(hipMemsetAsync(h->m.mem.acc, 0, 24, s));
  hipEventRecord(c.e0, s);
  size_t set = 0;
  for (int i = 0; i < count; i += c.max_batch, ++set) {
    const int B = std::min(c.max_batch, count - i);
    if (int rc = enqueue_batch(h, B, nullptr, first + i, false, 1.0, 1.0, set)) return rc;
  }
  c.nsets = set;
  h->last = nnmpc_train::LAST_SUMS; h->last_tan = tan_active(c); h->last_den = (double)count * c.nu;
  hipEventRecord(c.e1, s);
  double sum = 0.0;
  if (int rc = read_doubles(c, h->m.mem.acc, &sum, 1)) return rc;
  *mse = sum / ((double)count * c.nu);
  return NNMPC_OK;
  GUARD_END
}

int nnmpc_train_get_weights(nnmpc_train* h, double* const* W, double* const* b) {
  GUARD_BEGIN
  if (!h || !W || !b) { set_error("nnmpc_train_get_weights: bad arguments"); return NNMPC_EINVAL; }
  return get_weights(h->c, h->m, W, b);
  GUARD_END
}

int nnmpc_train_set_weights(nnmpc_train* h, const double* const* W, const double* const* b) {
  GUARD_BEGIN
  if (!h || !W || !b) { set_error("nnmpc_train_set_weights: bad arguments"); return NNMPC_EINVAL; }
  return set_weights(__func__, h->c, h->m, W, b);
  GUARD_END
}

int nnmpc_train_snapshot(nnmpc_train* h) {
  if (!h) { set_error("nnmpc_train_snapshot: bad arguments"); return NNMPC_EINVAL; }
  HIPCHK(hipSetDevice(h->c.device));
  return copy_params(h->c, h->m, true);
}

int nnmpc_train_restore(nnmpc_train* h) {
  if (!h) { set_error("nnmpc_train_restore: bad arguments"); return NNMPC_EINVAL; }
  HIPCHK(hipSetDevice(h->c.device));
  return copy_params(h->c, h->m, false);
}

int nnmpc_train_last_ms(nnmpc_train* h, double* gemm_ms, double* total_ms) {
  if (!h) { set_error("nnmpc_train_last_ms: bad arguments"); return NNMPC_EINVAL; }
  return last_ms(h->c, gemm_ms, total_ms);
}

int nnmpc_train_dw_slices(nnmpc_train* h, int32_t* slices) {
  if (!h || !slices) { set_error("nnmpc_train_dw_slices: bad arguments"); return NNMPC_EINVAL; }
  for (int l = 0; l < h->c.L; ++l) slices[l] = h->slices[l];
  return NNMPC_OK;
}

int nnmpc_train_padding_max(nnmpc_train* h, double* maxabs) {
  GUARD_BEGIN
  if (!h || !maxabs) { set_error("nnmpc_train_padding_max: bad arguments"); return NNMPC_EINVAL; }
  HIPCHK(hipSetDevice(h->c.device));
  HIPCHK(stream_sync(h->c.stream));
  *maxabs = 0.0;
  return padding_scan(h->c, h->m, maxabs);
  GUARD_END
}

}  // extern "C"
