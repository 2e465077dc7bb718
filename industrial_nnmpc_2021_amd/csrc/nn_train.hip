// Training step of the structured NN controller for gfx950 (f32 storage and accumulation, losses summed in fp64):
//   pred = us + MLP([x, (uprev), xs, us]) - MLP([xs, (us), xs, us]),  loss = mean (pred - u)^2,  Adam.
// Counterpart of train.py's torch step (RegulatorModel + torch.optim.Adam), reference cdu_train.py:40-62.
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
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <math.h>
#include <vector>
#include <algorithm>
#include <new>
#include "../../include/nnmpc.h"
#include "gemm_kernels.h"
#include "tile_gemm_tn.h"
#include "nn_train_dev.h"
#include "common.h"

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

__global__ void train_cvt_k(float* __restrict__ d, const double* __restrict__ s, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n; i += (size_t)gridDim.x * blockDim.x) d[i] = (float)s[i];
}

}  // namespace

struct nnmpc_train {
  int device = 0, L = 0;
  std::vector<int> dims, kpad, npad, slices;                // slices: of the last backward pass, per layer
  int nx = 0, nu = 0, with_uprev = 0, force_slices = 0, num_cus = 0;
  int max_batch = 0, cap_batch = 0;                         // the caller's limit (what B is checked against); rounded up to 128: the workspaces
  double lr = 0, beta1 = 0, beta2 = 0, eps = 0;
  long t = 0;                                               // Adam steps taken
  std::vector<float*> Wt, Wk, b, mW, vW, mb, vb, sWt, sWk, sb;   // Wt [npad][kpad], Wk [kpad][npad]; s*: the snapshot
  std::vector<float*> planes, bplanes, gW, gb;              // dW / db partial planes, summed gradients (grad only)
  std::vector<int> max_slices;
  std::vector<float*> act;                                  // L + 1 activations [2 max_batch][width]
  float* dz[2] = {nullptr, nullptr};
  int maxw = 0;
  int n = 0;                                                // dataset rows
  float *dx = nullptr, *dup = nullptr, *dxs = nullptr, *dus = nullptr, *du = nullptr;
  int* idx = nullptr; size_t idx_cap = 0;
  int* stage[2] = {nullptr, nullptr};                       // pinned copies of the caller's row list, used in turn
  hipEvent_t stage_done[2] = {nullptr, nullptr};            // the upload out of stage[k] has finished
  size_t stage_cap[2] = {0, 0}; int stage_turn = 0;
  double *partial = nullptr, *loss = nullptr, *acc = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  std::vector<hipEvent_t> ev;                               // 4 per step of the last call: forward GEMMs, backward
  size_t nsets = 0;
  std::vector<void*> allocs;
};

namespace {
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { set_error("%s: %s", #x, hipGetErrorString(e_)); return NNMPC_EHIP; } } while (0)
#define GUARD_BEGIN try {
#define GUARD_END } catch (const std::bad_alloc&) { set_error("%s: out of host memory", __func__); return NNMPC_ENOMEM; } \
                    catch (...) { set_error("%s: unexpected exception", __func__); return NNMPC_EHIP; }

template <class T>
int tr_alloc(nnmpc_train* h, T** p, size_t count) {
  void* q = nullptr;
  count = std::max<size_t>(count, 1);
  if (hipMalloc(&q, count * sizeof(T)) != hipSuccess) { set_error("hipMalloc(%zu) failed", count * sizeof(T)); return NNMPC_ENOMEM; }
  if (hipMemset(q, 0, count * sizeof(T)) != hipSuccess) { hipFree(q); set_error("hipMemset failed"); return NNMPC_EHIP; }
  h->allocs.push_back(q);
  *p = (T*)q;
  return 0;
}
void tr_free(nnmpc_train* h, void* p) {
  if (!p) return;
  auto it = std::find(h->allocs.begin(), h->allocs.end(), p);
  if (it != h->allocs.end()) h->allocs.erase(it);
  hipFree(p);
}

template <int NB, bool RELU, bool BIAS>
void launch_fwd(hipStream_t s, float* C, size_t ldc, const float* A, size_t lda, const float* Wt, size_t ldb, int M, int N,
                int K, const float* bias) {
  hipLaunchKernelGGL((gemm_nt_f32_k<NB, RELU, BIAS>), dim3(N / NB, M / NB), dim3(256), TileCfg<NB>::LDS_FLOATS * 4, s,
                     C, ldc, A, lda, Wt, ldb, K, bias);
}

// The slice rule of nn_train_dev.h at this handle's device and override.
int dw_slices_wanted(const nnmpc_train* h, int M, int tiles) {   // non-decreasing in M: its value at 2 max_batch sizes the planes
  return nnmpc::dw_slices_wanted(h->force_slices, h->num_cus, M, tiles);
}
int dw_slices(const nnmpc_train* h, int M, int tiles, int* slice_rows) {
  return nnmpc::dw_slices(h->force_slices, h->num_cus, M, tiles, slice_rows);
}

// Host Keras-order weights -> the padded device images (both layouts) of layer l.
int upload_layer(nnmpc_train* h, int l, const double* W, const double* b) {
  const int kp = h->kpad[l], np_ = h->npad[l], di = h->dims[l], dn = h->dims[l + 1];
  std::vector<float> wt((size_t)np_ * kp, 0.f), wk((size_t)kp * np_, 0.f), bb(np_, 0.f);
  for (int i = 0; i < di; ++i)
    for (int o = 0; o < dn; ++o) {
      const float w = (float)W[(size_t)i * dn + o];
      wt[(size_t)o * kp + i] = w; wk[(size_t)i * np_ + o] = w;
    }
  if (l < h->L - 1) for (int o = 0; o < dn; ++o) bb[o] = (float)b[o];
  HIPCHK(hipMemcpy(h->Wt[l], wt.data(), wt.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->Wk[l], wk.data(), wk.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->b[l], bb.data(), bb.size() * 4, hipMemcpyHostToDevice));
  return NNMPC_OK;
}

struct EvSet { hipEvent_t f0, f1, b0, b1; };
int ev_set(nnmpc_train* h, size_t i, EvSet* e) {
  while (h->ev.size() < 4 * (i + 1)) { hipEvent_t x; HIPCHK(hipEventCreate(&x)); h->ev.push_back(x); }
  *e = EvSet{h->ev[4 * i], h->ev[4 * i + 1], h->ev[4 * i + 2], h->ev[4 * i + 3]};
  return NNMPC_OK;
}

// Gather, forward, output kernel and (backward) the gradient planes of one batch on the handle's stream; no host wait.
// idx: device row list (nullptr: rows first .. first + B - 1).  The loss goes to *h->loss = loss_scale * sum of squares and
// *h->acc += acc_w * that.
int enqueue_batch(nnmpc_train* h, int B, const int* idx, int first, bool backward, double loss_scale, double acc_w, size_t set) {
  hipStream_t s = h->stream;
  const int L = h->L, Bp = ((B + 127) / 128) * 128, M = 2 * Bp;
  EvSet e;
  if (int rc = ev_set(h, set, &e)) return rc;
  hipLaunchKernelGGL(train_gather_k, dim3(std::min(Bp, 2048)), dim3(128), 0, s, h->act[0], h->kpad[0], Bp, B, h->nx, h->nu,
                     h->with_uprev, h->dx, h->dup, h->dxs, h->dus, idx, first);
  hipEventRecord(e.f0, s);
  for (int l = 0; l < L; ++l) {
    const int K = h->kpad[l], N = h->npad[l];
    const bool last = l == L - 1;
    if (N % 128 == 0) {
      if (last) launch_fwd<128, false, false>(s, h->act[l + 1], N, h->act[l], K, h->Wt[l], K, M, N, K, nullptr);
      else launch_fwd<128, true, true>(s, h->act[l + 1], N, h->act[l], K, h->Wt[l], K, M, N, K, h->b[l]);
    } else {
      if (last) launch_fwd<64, false, false>(s, h->act[l + 1], N, h->act[l], K, h->Wt[l], K, M, N, K, nullptr);
      else launch_fwd<64, true, true>(s, h->act[l + 1], N, h->act[l], K, h->Wt[l], K, M, N, K, h->b[l]);
    }
  }
  hipEventRecord(e.f1, s);
  const int ldo = h->npad[L - 1];
  float* dzc = backward ? h->dz[0] : nullptr;
  hipLaunchKernelGGL(train_output_k, dim3(Bp / 64), dim3(256), 0, s, dzc, h->act[L], ldo, Bp, B, h->nu, h->dus, h->du, idx,
                     first, (float)(2.0 / ((double)B * h->nu)), h->partial);
  hipLaunchKernelGGL(train_loss_finish_k, dim3(1), dim3(64), 0, s, h->partial, Bp / 64, loss_scale, acc_w, h->loss, h->acc);
  hipEventRecord(e.b0, s);
  if (backward) {
    int cur = 0;
    for (int l = L - 1; l >= 0; --l) {
      const int K = h->kpad[l], N = h->npad[l];
      const float* dZ = h->dz[cur];
      const bool big = N % 128 == 0 && K % 128 == 0;
      const int nb = big ? 128 : 64;
      int slice_rows = 0;
      const int S = dw_slices(h, M, (N / nb) * (K / nb), &slice_rows);
      if (S > h->max_slices[l]) { set_error("nnmpc_train: %d dW slices for layer %d, planes for %d", S, l, h->max_slices[l]); return NNMPC_EINVAL; }
      h->slices[l] = S;
      const size_t plane = (size_t)N * K;
      if (big)
        hipLaunchKernelGGL(gemm_tn_f32_k<128>, dim3(K / 128, N / 128, S), dim3(256), TileCfgTN<128>::LDS_FLOATS * 4, s,
                           h->planes[l], plane, (size_t)K, dZ, (size_t)N, h->act[l], (size_t)K, M, slice_rows);
      else
        hipLaunchKernelGGL(gemm_tn_f32_k<64>, dim3(K / 64, N / 64, S), dim3(256), TileCfgTN<64>::LDS_FLOATS * 4, s,
                           h->planes[l], plane, (size_t)K, dZ, (size_t)N, h->act[l], (size_t)K, M, slice_rows);
      if (l < L - 1)
        hipLaunchKernelGGL(train_colsum_k, dim3(N / 64, M / 128), dim3(256), 0, s, h->bplanes[l], dZ, N);
      if (l > 0) {                                           // dZ_{l-1} [M][K] = (dZ_l [M][N] Wk_l [K][N]') * mask(A_l input = act[l])
        if (K % 128 == 0)
          hipLaunchKernelGGL(gemm_nt_mask_k<128>, dim3(K / 128, M / 128), dim3(256), TileCfg<128>::LDS_FLOATS * 4, s,
                             h->dz[cur ^ 1], (size_t)K, dZ, (size_t)N, h->Wk[l], (size_t)N, N, h->act[l]);
        else
          hipLaunchKernelGGL(gemm_nt_mask_k<64>, dim3(K / 64, M / 64), dim3(256), TileCfg<64>::LDS_FLOATS * 4, s,
                             h->dz[cur ^ 1], (size_t)K, dZ, (size_t)N, h->Wk[l], (size_t)N, N, h->act[l]);
        cur ^= 1;
      }
    }
  }
  hipEventRecord(e.b1, s);
  return NNMPC_OK;
}

// The Adam update of every tensor from the planes of the last backward pass of a batch of Bp padded rows.
void enqueue_adam(nnmpc_train* h, int Bp) {
  ++h->t;
  const AdamCoef k = adam_coef(h->lr, h->beta1, h->beta2, h->eps, h->t);
  for (int l = 0; l < h->L; ++l) {
    const int K = h->kpad[l], N = h->npad[l];
    hipLaunchKernelGGL(train_adam_w_k, dim3(K / 64, N / 64), dim3(256), 0, h->stream, h->Wt[l], h->Wk[l], h->mW[l], h->vW[l],
                       h->planes[l], (size_t)N * K, h->slices[l], K, N, k);
    if (l < h->L - 1)
      hipLaunchKernelGGL(train_adam_b_k, dim3((N + 255) / 256), dim3(256), 0, h->stream, h->b[l], h->mb[l], h->vb[l],
                         h->bplanes[l], N, 2 * Bp / 128, k);
  }
}

int check_rows(const nnmpc_train* h, const char* who, int count, const int32_t* rows) {
  for (int i = 0; i < count; ++i)
    if (rows[i] < 0 || rows[i] >= h->n) { set_error("%s: row index %d at position %d outside [0, %d)", who, rows[i], i, h->n); return NNMPC_EINVAL; }
  return NNMPC_OK;
}
int check_batch(const nnmpc_train* h, const char* who, int B) {
  if (!h->dx) { set_error("%s: no dataset (call nnmpc_train_set_data first)", who); return NNMPC_EINVAL; }
  if (B < 1 || B > h->max_batch) { set_error("%s: batch of %d rows, max_batch is %d", who, B, h->max_batch); return NNMPC_EINVAL; }
  return NNMPC_OK;
}
// The caller's row list goes through a pinned buffer of the handle, so `rows` may be reused as soon as the call returns
// and the upload is a true asynchronous copy.  Two buffers are used in turn; before one is overwritten the host waits for
// the upload that last read it (two calls back), never for the kernels of the previous call.
int upload_rows(nnmpc_train* h, int count, const int32_t* rows) {
  if ((size_t)count > h->idx_cap) {
    tr_free(h, h->idx); h->idx = nullptr; h->idx_cap = 0;
    if (int rc = tr_alloc(h, &h->idx, (size_t)count)) return rc;
    h->idx_cap = count;
  }
  const int k = h->stage_turn;
  h->stage_turn ^= 1;
  if (!h->stage_done[k]) HIPCHK(hipEventCreateWithFlags(&h->stage_done[k], hipEventDisableTiming));
  else HIPCHK(hipEventSynchronize(h->stage_done[k]));
  if ((size_t)count > h->stage_cap[k]) {
    if (h->stage[k]) { hipHostFree(h->stage[k]); h->stage[k] = nullptr; h->stage_cap[k] = 0; }
    void* q = nullptr;
    if (hipHostMalloc(&q, (size_t)count * 4, hipHostMallocDefault) != hipSuccess) { set_error("hipHostMalloc(%zu) failed", (size_t)count * 4); return NNMPC_ENOMEM; }
    h->stage[k] = (int*)q; h->stage_cap[k] = count;
  }
  memcpy(h->stage[k], rows, (size_t)count * 4);
  HIPCHK(hipMemcpyAsync(h->idx, h->stage[k], (size_t)count * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipEventRecord(h->stage_done[k], h->stream));
  return NNMPC_OK;
}
int read_loss(nnmpc_train* h, const double* src, double* out) {
  HIPCHK(hipMemcpyAsync(out, src, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(stream_sync(h->stream));
  HIPCHK(hipGetLastError());
  return NNMPC_OK;
}
}  // namespace

extern "C" {

int nnmpc_train_destroy(nnmpc_train* h) {
  if (!h) return NNMPC_OK;
  hipSetDevice(h->device);
  hipDeviceSynchronize();
  for (void* p : h->allocs) hipFree(p);
  for (int k = 0; k < 2; ++k) {
    if (h->stage[k]) hipHostFree(h->stage[k]);
    if (h->stage_done[k]) hipEventDestroy(h->stage_done[k]);
  }
  if (h->e0) hipEventDestroy(h->e0);
  if (h->e1) hipEventDestroy(h->e1);
  for (hipEvent_t e : h->ev) hipEventDestroy(e);
  if (h->stream) hipStreamDestroy(h->stream);
  delete h;
  return NNMPC_OK;
}

int nnmpc_train_create(nnmpc_train** out, int32_t nlayers, const int32_t* dims, const double* const* W,
                       const double* const* b, int32_t nx, int32_t nu, int32_t with_uprev, int32_t max_batch,
                       double lr, double beta1, double beta2, double eps) {
  GUARD_BEGIN
  if (!out || nlayers < 1 || !dims || !W || !b || nx <= 0 || nu <= 0 || max_batch < 1) { set_error("nnmpc_train_create: bad arguments"); return NNMPC_EINVAL; }
  const int din = 2 * nx + (with_uprev ? 2 : 1) * nu;
  if (dims[0] != din || dims[nlayers] != nu) { set_error("nnmpc_train_create: dims[0]=%d (want %d), dims[L]=%d (want %d)", dims[0], din, dims[nlayers], nu); return NNMPC_EINVAL; }
  for (int l = 0; l <= nlayers; ++l)
    if (dims[l] < 1) { set_error("nnmpc_train_create: dims[%d]=%d", l, dims[l]); return NNMPC_EINVAL; }
  for (int l = 0; l < nlayers; ++l)
    if (!W[l] || (l < nlayers - 1 && !b[l])) { set_error("nnmpc_train_create: missing weights or bias of layer %d", l); return NNMPC_EINVAL; }
  if (!(lr > 0) || !(beta1 >= 0 && beta1 < 1) || !(beta2 >= 0 && beta2 < 1) || !(eps > 0)) { set_error("nnmpc_train_create: bad Adam parameters (lr > 0, 0 <= beta < 1, eps > 0: with eps = 0 an entry whose gradient is exactly zero, all padding included, would become 0 / 0)"); return NNMPC_EINVAL; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { set_error("nnmpc_train_create: no HIP device available (no CPU fallback)"); return NNMPC_EHIP; }
  struct Destroy { void operator()(nnmpc_train* p) const { nnmpc_train_destroy(p); } };
  std::unique_ptr<nnmpc_train, Destroy> guard(new nnmpc_train());   // released into *out at the end; destroyed on any other way out
  nnmpc_train* h = guard.get();
  HIPCHK(hipGetDevice(&h->device));
  HIPCHK(hipDeviceGetAttribute(&h->num_cus, hipDeviceAttributeMultiprocessorCount, h->device));
  if (h->num_cus < 1) { set_error("nnmpc_train_create: device reports %d compute units", h->num_cus); return NNMPC_EHIP; }
  h->L = nlayers; h->nx = nx; h->nu = nu; h->with_uprev = with_uprev != 0;
  h->max_batch = max_batch;
  h->cap_batch = ((max_batch + 127) / 128) * 128;
  h->lr = lr; h->beta1 = beta1; h->beta2 = beta2; h->eps = eps;
  h->dims.assign(dims, dims + nlayers + 1);
  if (const char* e = getenv("NNMPC_TRAIN_DW_SLICES")) h->force_slices = std::max(0, atoi(e));   // tests: several slices on a small batch
  int rc = 0;
  if (hipStreamCreate(&h->stream) != hipSuccess || hipEventCreate(&h->e0) != hipSuccess || hipEventCreate(&h->e1) != hipSuccess) {
    set_error("nnmpc_train_create: stream / event creation failed"); return NNMPC_EHIP;
  }
  HIPCHK(hipFuncSetAttribute((const void*)gemm_nt_f32_k<128, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, TileCfg<128>::LDS_FLOATS * 4));
  HIPCHK(hipFuncSetAttribute((const void*)gemm_nt_f32_k<128, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, TileCfg<128>::LDS_FLOATS * 4));
  HIPCHK(hipFuncSetAttribute((const void*)gemm_nt_mask_k<128>, hipFuncAttributeMaxDynamicSharedMemorySize, TileCfg<128>::LDS_FLOATS * 4));
  HIPCHK(hipFuncSetAttribute((const void*)gemm_tn_f32_k<128>, hipFuncAttributeMaxDynamicSharedMemorySize, TileCfgTN<128>::LDS_FLOATS * 4));
  const size_t MB = h->cap_batch, Mmax = 2 * MB;
  for (int l = 0; l < nlayers && !rc; ++l) {
    const int kp = l == 0 ? ((dims[0] + 63) / 64) * 64 : h->npad[l - 1];
    const int np_ = dims[l + 1] > 64 ? ((dims[l + 1] + 127) / 128) * 128 : 64;   // as nnmpc_nn_create
    h->kpad.push_back(kp); h->npad.push_back(np_);
    h->maxw = std::max(h->maxw, std::max(kp, np_));
    const size_t plane = (size_t)np_ * kp;
    const int nb = (np_ % 128 == 0 && kp % 128 == 0) ? 128 : 64;
    const int smax = dw_slices_wanted(h, (int)Mmax, (np_ / nb) * (kp / nb));
    h->max_slices.push_back(smax); h->slices.push_back(1);
    float* p[12] = {nullptr};
    const size_t cnt[12] = {plane, plane, (size_t)np_, plane, plane, (size_t)np_, (size_t)np_, plane, plane, (size_t)np_, plane, (size_t)np_};
    for (int j = 0; j < 12 && !rc; ++j) rc = tr_alloc(h, &p[j], cnt[j]);
    float *pl = nullptr, *bpl = nullptr;
    if (!rc) rc = tr_alloc(h, &pl, plane * smax);
    if (!rc) rc = tr_alloc(h, &bpl, (size_t)np_ * (Mmax / 128));
    h->Wt.push_back(p[0]); h->Wk.push_back(p[1]); h->b.push_back(p[2]); h->mW.push_back(p[3]); h->vW.push_back(p[4]);
    h->mb.push_back(p[5]); h->vb.push_back(p[6]); h->sWt.push_back(p[7]); h->sWk.push_back(p[8]); h->sb.push_back(p[9]);
    h->gW.push_back(p[10]); h->gb.push_back(p[11]); h->planes.push_back(pl); h->bplanes.push_back(bpl);
    if (!rc) rc = upload_layer(h, l, W[l], b[l]);
  }
  for (int l = 0; l <= nlayers && !rc; ++l) {
    float* a = nullptr;
    rc = tr_alloc(h, &a, Mmax * (size_t)(l == 0 ? h->kpad[0] : h->npad[l - 1]));
    h->act.push_back(a);
  }
  if (!rc) rc = tr_alloc(h, &h->dz[0], Mmax * h->maxw);
  if (!rc) rc = tr_alloc(h, &h->dz[1], Mmax * h->maxw);
  if (!rc) rc = tr_alloc(h, &h->partial, MB / 64);
  if (!rc) rc = tr_alloc(h, &h->loss, 1);
  if (!rc) rc = tr_alloc(h, &h->acc, 1);
  if (rc) return rc;
  for (int l = 0; l < nlayers; ++l) {                      // the snapshot starts as the initial weights
    HIPCHK(hipMemcpy(h->sWt[l], h->Wt[l], (size_t)h->npad[l] * h->kpad[l] * 4, hipMemcpyDeviceToDevice));
    HIPCHK(hipMemcpy(h->sWk[l], h->Wk[l], (size_t)h->npad[l] * h->kpad[l] * 4, hipMemcpyDeviceToDevice));
    HIPCHK(hipMemcpy(h->sb[l], h->b[l], (size_t)h->npad[l] * 4, hipMemcpyDeviceToDevice));
  }
  *out = guard.release();
  return NNMPC_OK;
  GUARD_END
}

int nnmpc_train_set_data(nnmpc_train* h, int32_t n, const double* x, const double* uprev, const double* xs, const double* us,
                         const double* u, int32_t ptr_kind) {
  GUARD_BEGIN
  if (!h || n < 1 || !x || !xs || !us || !u) { set_error("nnmpc_train_set_data: bad arguments"); return NNMPC_EINVAL; }
  if (h->with_uprev && !uprev) { set_error("nnmpc_train_set_data: the network takes uprev, none given"); return NNMPC_EINVAL; }
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(stream_sync(h->stream));
  for (float** p : {&h->dx, &h->dup, &h->dxs, &h->dus, &h->du}) { tr_free(h, *p); *p = nullptr; }
  h->n = 0;
  struct { float** d; const double* s; int w; } col[5] = {{&h->dx, x, h->nx}, {&h->dup, h->with_uprev ? uprev : nullptr, h->nu},
                                                          {&h->dxs, xs, h->nx}, {&h->dus, us, h->nu}, {&h->du, u, h->nu}};
  std::vector<float> tmp;
  for (auto& c : col) {
    if (!c.s) continue;
    const size_t cnt = (size_t)n * c.w;
    if (int rc = tr_alloc(h, c.d, cnt)) return rc;
    if (ptr_kind == NNMPC_HOST) {
      tmp.resize(cnt);
      for (size_t i = 0; i < cnt; ++i) tmp[i] = (float)c.s[i];
      HIPCHK(hipMemcpy(*c.d, tmp.data(), cnt * 4, hipMemcpyHostToDevice));
    } else {
      hipLaunchKernelGGL(train_cvt_k, dim3(1024), dim3(256), 0, h->stream, *c.d, c.s, cnt);
    }
  }
  HIPCHK(stream_sync(h->stream));
  HIPCHK(hipGetLastError());
  h->n = n;
  return NNMPC_OK;
  GUARD_END
}

int nnmpc_train_grad(nnmpc_train* h, int32_t B, const int32_t* rows, double* loss, double* const* gW, double* const* gb) {
  GUARD_BEGIN
  if (!h || !rows) { set_error("nnmpc_train_grad: bad arguments"); return NNMPC_EINVAL; }
  if (int rc = check_batch(h, "nnmpc_train_grad", B)) return rc;
  if (int rc = check_rows(h, "nnmpc_train_grad", B, rows)) return rc;
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  if (int rc = upload_rows(h, B, rows)) return rc;
  hipEventRecord(h->e0, s);
  if (int rc = enqueue_batch(h, B, h->idx, 0, true, 1.0 / ((double)B * h->nu), 0.0, 0)) return rc;
  h->nsets = 1;
  const int Bp = ((B + 127) / 128) * 128;
  for (int l = 0; l < h->L; ++l) {
    const size_t plane = (size_t)h->npad[l] * h->kpad[l];
    hipLaunchKernelGGL(train_plane_sum_k, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, s, h->gW[l], h->planes[l], plane, h->slices[l]);
    if (l < h->L - 1)
      hipLaunchKernelGGL(train_plane_sum_k, dim3((h->npad[l] + 255) / 256), dim3(256), 0, s, h->gb[l], h->bplanes[l], (size_t)h->npad[l], 2 * Bp / 128);
  }
  hipEventRecord(h->e1, s);
  double lv = 0.0;
  if (int rc = read_loss(h, h->loss, &lv)) return rc;
  if (loss) *loss = lv;
  std::vector<float> tmp;
  for (int l = 0; l < h->L; ++l) {
    const int kp = h->kpad[l], np_ = h->npad[l], di = h->dims[l], dn = h->dims[l + 1];
    if (gW && gW[l]) {
      tmp.resize((size_t)np_ * kp);
      HIPCHK(hipMemcpy(tmp.data(), h->gW[l], tmp.size() * 4, hipMemcpyDeviceToHost));
      for (int i = 0; i < di; ++i)
        for (int o = 0; o < dn; ++o) gW[l][(size_t)i * dn + o] = (double)tmp[(size_t)o * kp + i];
    }
    if (gb && l < h->L - 1 && gb[l]) {
      tmp.resize(np_);
      HIPCHK(hipMemcpy(tmp.data(), h->gb[l], (size_t)np_ * 4, hipMemcpyDeviceToHost));
      for (int o = 0; o < dn; ++o) gb[l][o] = (double)tmp[o];
    }
  }
  return NNMPC_OK;
  GUARD_END
}

int nnmpc_train_step(nnmpc_train* h, int32_t B, const int32_t* rows, double* loss) {
  GUARD_BEGIN
  if (!h || !rows) { set_error("nnmpc_train_step: bad arguments"); return NNMPC_EINVAL; }
  if (int rc = check_batch(h, "nnmpc_train_step", B)) return rc;
  if (int rc = check_rows(h, "nnmpc_train_step", B, rows)) return rc;
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  if (int rc = upload_rows(h, B, rows)) return rc;
  hipEventRecord(h->e0, s);
  if (int rc = enqueue_batch(h, B, h->idx, 0, true, 1.0 / ((double)B * h->nu), 0.0, 0)) return rc;
  h->nsets = 1;
  enqueue_adam(h, ((B + 127) / 128) * 128);
  hipEventRecord(h->e1, s);
  if (loss) return read_loss(h, h->loss, loss);
  return NNMPC_OK;
  GUARD_END
}

int nnmpc_train_epoch(nnmpc_train* h, int32_t nrows, const int32_t* perm, int32_t batch, double* loss) {
  GUARD_BEGIN
  if (!h || !perm || nrows < 1) { set_error("nnmpc_train_epoch: bad arguments"); return NNMPC_EINVAL; }
  if (int rc = check_batch(h, "nnmpc_train_epoch", batch)) return rc;
  if (int rc = check_rows(h, "nnmpc_train_epoch", nrows, perm)) return rc;
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  if (int rc = upload_rows(h, nrows, perm)) return rc;
  HIPCHK(hipMemsetAsync(h->acc, 0, 8, s));
  hipEventRecord(h->e0, s);
  size_t set = 0;
  for (int i = 0; i < nrows; i += batch, ++set) {
    const int B = std::min(batch, nrows - i);              // the last batch is the short one
    if (int rc = enqueue_batch(h, B, h->idx + i, 0, true, 1.0 / ((double)B * h->nu), (double)B, set)) return rc;
    enqueue_adam(h, ((B + 127) / 128) * 128);
  }
  h->nsets = set;
  hipEventRecord(h->e1, s);
  double sum = 0.0;
  if (int rc = read_loss(h, h->acc, &sum)) return rc;
  if (loss) *loss = sum / (double)nrows;
  return NNMPC_OK;
  GUARD_END
}

int nnmpc_train_eval(nnmpc_train* h, int32_t first, int32_t count, double* mse) {
  GUARD_BEGIN
  if (!h || !mse) { set_error("nnmpc_train_eval: bad arguments"); return NNMPC_EINVAL; }
  if (!h->dx) { set_error("nnmpc_train_eval: no dataset (call nnmpc_train_set_data first)"); return NNMPC_EINVAL; }
  if (first < 0 || count < 1 || (int64_t)first + count > h->n) { set_error("nnmpc_train_eval: rows [%d, %d + %d) outside [0, %d)", first, first, count, h->n); return NNMPC_EINVAL; }
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  HIPCHK(hipMemsetAsync(h->acc, 0, 8, s));
  hipEventRecord(h->e0, s);
  size_t set = 0;
  for (int i = 0; i < count; i += h->max_batch, ++set) {
    const int B = std::min(h->max_batch, count - i);
    if (int rc = enqueue_batch(h, B, nullptr, first + i, false, 1.0, 1.0, set)) return rc;
  }
  h->nsets = set;
  hipEventRecord(h->e1, s);
  double sum = 0.0;
  if (int rc = read_loss(h, h->acc, &sum)) return rc;
  *mse = sum / ((double)count * h->nu);
  return NNMPC_OK;
  GUARD_END
}

int nnmpc_train_get_weights(nnmpc_train* h, double* const* W, double* const* b) {
  GUARD_BEGIN
  if (!h || !W || !b) { set_error("nnmpc_train_get_weights: bad arguments"); return NNMPC_EINVAL; }
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(stream_sync(h->stream));
  std::vector<float> tmp;
  for (int l = 0; l < h->L; ++l) {
    const int kp = h->kpad[l], np_ = h->npad[l], di = h->dims[l], dn = h->dims[l + 1];
    if (W[l]) {
      tmp.resize((size_t)np_ * kp);
      HIPCHK(hipMemcpy(tmp.data(), h->Wt[l], tmp.size() * 4, hipMemcpyDeviceToHost));
      for (int i = 0; i < di; ++i)
        for (int o = 0; o < dn; ++o) W[l][(size_t)i * dn + o] = (double)tmp[(size_t)o * kp + i];
    }
    if (l < h->L - 1 && b[l]) {
      tmp.resize(np_);
      HIPCHK(hipMemcpy(tmp.data(), h->b[l], (size_t)np_ * 4, hipMemcpyDeviceToHost));
      for (int o = 0; o < dn; ++o) b[l][o] = (double)tmp[o];
    }
  }
  return NNMPC_OK;
  GUARD_END
}

int nnmpc_train_set_weights(nnmpc_train* h, const double* const* W, const double* const* b) {
  GUARD_BEGIN
  if (!h || !W || !b) { set_error("nnmpc_train_set_weights: bad arguments"); return NNMPC_EINVAL; }
  for (int l = 0; l < h->L; ++l)
    if (!W[l] || (l < h->L - 1 && !b[l])) { set_error("nnmpc_train_set_weights: missing weights or bias of layer %d", l); return NNMPC_EINVAL; }
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(stream_sync(h->stream));
  for (int l = 0; l < h->L; ++l)
    if (int rc = upload_layer(h, l, W[l], b[l])) return rc;
  return NNMPC_OK;
  GUARD_END
}

static int copy_weights(nnmpc_train* h, std::vector<float*>& dWt, std::vector<float*>& dWk, std::vector<float*>& db,
                        std::vector<float*>& sWt, std::vector<float*>& sWk, std::vector<float*>& sb) {
  HIPCHK(hipSetDevice(h->device));
  for (int l = 0; l < h->L; ++l) {
    const size_t plane = (size_t)h->npad[l] * h->kpad[l] * 4;
    HIPCHK(hipMemcpyAsync(dWt[l], sWt[l], plane, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(dWk[l], sWk[l], plane, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(db[l], sb[l], (size_t)h->npad[l] * 4, hipMemcpyDeviceToDevice, h->stream));
  }
  return NNMPC_OK;
}

int nnmpc_train_snapshot(nnmpc_train* h) {
  if (!h) { set_error("nnmpc_train_snapshot: bad arguments"); return NNMPC_EINVAL; }
  return copy_weights(h, h->sWt, h->sWk, h->sb, h->Wt, h->Wk, h->b);
}

int nnmpc_train_restore(nnmpc_train* h) {
  if (!h) { set_error("nnmpc_train_restore: bad arguments"); return NNMPC_EINVAL; }
  return copy_weights(h, h->Wt, h->Wk, h->b, h->sWt, h->sWk, h->sb);
}

int nnmpc_train_last_ms(nnmpc_train* h, double* gemm_ms, double* total_ms) {
  if (!h) { set_error("nnmpc_train_last_ms: bad arguments"); return NNMPC_EINVAL; }
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(stream_sync(h->stream));
  double g = 0.0;
  float ms = 0.f;
  for (size_t i = 0; i < h->nsets && 4 * i + 3 < h->ev.size(); ++i) {
    if (hipEventElapsedTime(&ms, h->ev[4 * i], h->ev[4 * i + 1]) == hipSuccess) g += ms;
    if (hipEventElapsedTime(&ms, h->ev[4 * i + 2], h->ev[4 * i + 3]) == hipSuccess) g += ms;
  }
  ms = 0.f;
  if (h->nsets) hipEventElapsedTime(&ms, h->e0, h->e1);
  if (gemm_ms) *gemm_ms = g;
  if (total_ms) *total_ms = ms;
  return NNMPC_OK;
}

int nnmpc_train_dw_slices(nnmpc_train* h, int32_t* slices) {
  if (!h || !slices) { set_error("nnmpc_train_dw_slices: bad arguments"); return NNMPC_EINVAL; }
  for (int l = 0; l < h->L; ++l) slices[l] = h->slices[l];
  return NNMPC_OK;
}

int nnmpc_train_padding_max(nnmpc_train* h, double* maxabs) {
  GUARD_BEGIN
  if (!h || !maxabs) { set_error("nnmpc_train_padding_max: bad arguments"); return NNMPC_EINVAL; }
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(stream_sync(h->stream));
  double mx = 0.0;
  std::vector<float> tmp;
  auto fold = [&](float v) { const double a = fabs((double)v); if (mx == mx && !(a <= mx)) mx = a; };   // a NaN in the padding counts, and stays
  for (int l = 0; l < h->L; ++l) {
    const int kp = h->kpad[l], np_ = h->npad[l], di = h->dims[l], dn = h->dims[l + 1];
    tmp.resize((size_t)np_ * kp);
    for (float* p : {h->Wt[l], h->mW[l], h->vW[l]}) {       // [out][in]
      HIPCHK(hipMemcpy(tmp.data(), p, tmp.size() * 4, hipMemcpyDeviceToHost));
      for (int o = 0; o < np_; ++o)
        for (int i = 0; i < kp; ++i) if (o >= dn || i >= di) fold(tmp[(size_t)o * kp + i]);
    }
    HIPCHK(hipMemcpy(tmp.data(), h->Wk[l], tmp.size() * 4, hipMemcpyDeviceToHost));   // [in][out]
    for (int i = 0; i < kp; ++i)
      for (int o = 0; o < np_; ++o) if (o >= dn || i >= di) fold(tmp[(size_t)i * np_ + o]);
    for (float* p : {h->b[l], h->mb[l], h->vb[l]}) {
      HIPCHK(hipMemcpy(tmp.data(), p, (size_t)np_ * 4, hipMemcpyDeviceToHost));
      for (int o = (l < h->L - 1 ? dn : 0); o < np_; ++o) fold(tmp[o]);
    }
  }
  *maxabs = mx;
  return NNMPC_OK;
  GUARD_END
}

}  // extern "C"
