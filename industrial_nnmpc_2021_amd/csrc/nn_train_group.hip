// A sweep of structured networks trained in lock step for gfx950: the step of nn_train.hip with the member network as a
// grid coordinate, so a layer of G networks is one launch (one per tile class present) instead of G.
//
// Members share nx, nu, with_uprev, the depth, max_batch, the Adam hyper-parameters and ONE f32 dataset; they differ in
// widths, weights, rows, Adam step count and snapshot.  In lock-step step k member g works on its batch k (B rows; B = 0:
// the member has run out of rows, or sits this call out, and every workgroup of its grid plane returns at once).
//
// A member's bytes do not depend on the rest of the group and equal what an nnmpc_train handle gives: every kernel here is
// the workgroup function of nn_train_dev.h that the single-network kernel runs, at the member's own block coordinates and
// with the member's own shapes (padding, tile class, dW slices from its own M and tile count); the scalars of a step (Adam
// bias corrections from the member's own t, loss scales) are computed on the host in double as nn_train.hip computes them
// and travel in a table uploaded once per call with the row lists.  No atomics, no hand-off between workgroups.
//
// Device tables:  GLayer [G][L] and GMember [G], written at create (pointers, padded K and N);  GStep [steps][G], per call.
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
#include "nn_train_dev.h"
#include "common.h"

using namespace nnmpc;

namespace {

struct GLayer {                                             // operands of layer l of member g
  float *Wt, *Wk, *b, *mW, *vW, *mb, *vb;                   // Wt [N][K], Wk [K][N]
  float *planes, *bplanes;                                  // dW / db partial planes
  float *ain, *aout;                                        // activations [2 cap_batch][K], [2 cap_batch][N]
  int K, N;                                                 // padded input / output width
};
struct GMember { float* dz[2]; double *partial, *loss, *acc; };
struct GStep {                                              // member g in lock-step step k
  AdamCoef k;                                               // from the member's own step count
  double loss_scale, acc_w;
  float gscale;
  int B, at, pad_;                                          // rows of the batch (0: inactive); position in the row lists, or first dataset row
};
struct GShape { int nx, nu, with_uprev, L, force_slices, num_cus; };
struct GData { const float *x, *uprev, *xs, *us, *u; };

__device__ __forceinline__ int pad128(int B) { return ((B + 127) / 128) * 128; }

// Grid (row blocks, G).
__global__ __launch_bounds__(128) void grp_gather_k(const GLayer* __restrict__ lay, const GStep* __restrict__ st, GShape sh,
                                                    GData d, const int* __restrict__ rows) {
  const int g = blockIdx.y, B = st[g].B;
  if (B == 0) return;
  const GLayer& ld = lay[(size_t)g * sh.L];
  train_gather_rows(ld.ain, ld.K, pad128(B), B, sh.nx, sh.nu, sh.with_uprev, d.x, d.uprev, d.xs, d.us,
                    rows ? rows + st[g].at : nullptr, st[g].at, blockIdx.x, gridDim.x);
}

// Layer l forward for the members whose N is in tile class NB.  Grid (max N / NB, max 2 Bp / NB, G); inside a member's own
// ntn x ntm extent the workgroup id is remapped as gemm_nt_f32_k remaps it (row panels of 8 back to back: a bijection of
// the extent; which workgroup computes a tile changes no sum).
template <int NB, bool RELU, bool BIAS>
__global__ __launch_bounds__(256) void grp_fwd_k(const GLayer* __restrict__ lay, const GStep* __restrict__ st, GShape sh, int l) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int g = blockIdx.z, B = st[g].B;
  if (B == 0) return;
  const GLayer& ld = lay[(size_t)g * sh.L + l];
  if ((ld.N % 128 == 0) != (NB == 128)) return;
  const int ntn = ld.N / NB, ntm = 2 * pad128(B) / NB;
  if ((int)blockIdx.x >= ntn || (int)blockIdx.y >= ntm) return;
  int tm, tn;
  {
    const int bid = blockIdx.x + ntn * blockIdx.y, full = (ntm >> 3) * 8 * ntn;
    if (bid < full) { const int sq = bid >> 3; tm = (sq / ntn) * 8 + (bid & 7); tn = sq % ntn; }
    else { const int rem = bid - full; tm = (ntm >> 3) * 8 + rem / ntn; tn = rem % ntn; }
  }
  train_fwd_tile<NB, RELU, BIAS>(ld.aout, ld.N, ld.ain, ld.K, ld.Wt, ld.K, ld.K, ld.b, tm, tn, lds);
}

// Grid (max Bp / 64, G).
__global__ __launch_bounds__(256) void grp_output_k(const GLayer* __restrict__ lay, const GMember* __restrict__ mem,
                                                    const GStep* __restrict__ st, GShape sh, GData d,
                                                    const int* __restrict__ rows, int backward) {
  const int g = blockIdx.y, B = st[g].B;
  if (B == 0) return;
  const int Bp = pad128(B);
  if ((int)blockIdx.x * 64 >= Bp) return;
  const GLayer& ld = lay[(size_t)g * sh.L + sh.L - 1];
  train_output_block(backward ? mem[g].dz[0] : nullptr, ld.aout, ld.N, Bp, B, sh.nu, d.us, d.u,
                     rows ? rows + st[g].at : nullptr, st[g].at, st[g].gscale, mem[g].partial, blockIdx.x);
}

// Grid (G): one thread per member.
__global__ void grp_loss_finish_k(const GMember* __restrict__ mem, const GStep* __restrict__ st) {
  const int g = blockIdx.x, B = st[g].B;
  if (threadIdx.x != 0 || B == 0) return;
  train_loss_finish(mem[g].partial, pad128(B) / 64, st[g].loss_scale, st[g].acc_w, mem[g].loss, mem[g].acc);
}

__device__ __forceinline__ int layer_slices(const GLayer& ld, const GShape& sh, int M, int* slice_rows) {
  const int nb = (ld.N % 128 == 0 && ld.K % 128 == 0) ? 128 : 64;
  return dw_slices(sh.force_slices, sh.num_cus, M, (ld.N / nb) * (ld.K / nb), slice_rows);
}

// dW planes of layer l for the members in tile class NB (N and K both multiples of 128, or not).
// Grid (max K / NB, max N / NB, G * smax): z = g * smax + slice; the slices are the member's own.
template <int NB>
__global__ __launch_bounds__(256) void grp_dw_k(const GLayer* __restrict__ lay, const GMember* __restrict__ mem,
                                                const GStep* __restrict__ st, GShape sh, int l, int cur, int smax) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int g = blockIdx.z / smax, s = blockIdx.z % smax, B = st[g].B;
  if (B == 0) return;
  const GLayer& ld = lay[(size_t)g * sh.L + l];
  if ((ld.N % 128 == 0 && ld.K % 128 == 0) != (NB == 128)) return;
  if ((int)blockIdx.x >= ld.K / NB || (int)blockIdx.y >= ld.N / NB) return;
  const int M = 2 * pad128(B);
  int slice_rows = 0;
  if (s >= layer_slices(ld, sh, M, &slice_rows)) return;
  train_tn_tile<NB>(ld.planes, (size_t)ld.N * ld.K, (size_t)ld.K, mem[g].dz[cur], (size_t)ld.N, ld.ain, (size_t)ld.K, M,
                    slice_rows, blockIdx.x, blockIdx.y, s, lds);
}

// Grid (max N / 64, max 2 Bp / 128, G).
__global__ __launch_bounds__(256) void grp_colsum_k(const GLayer* __restrict__ lay, const GMember* __restrict__ mem,
                                                    const GStep* __restrict__ st, GShape sh, int l, int cur) {
  const int g = blockIdx.z, B = st[g].B;
  if (B == 0) return;
  const GLayer& ld = lay[(size_t)g * sh.L + l];
  if ((int)blockIdx.x >= ld.N / 64 || (int)blockIdx.y >= 2 * pad128(B) / 128) return;
  train_colsum_block(ld.bplanes, mem[g].dz[cur], ld.N, blockIdx.x, blockIdx.y);
}

// dZ_{l-1} of layer l for the members whose K is in tile class NB.  Grid (max K / NB, max 2 Bp / NB, G).
template <int NB>
__global__ __launch_bounds__(256) void grp_da_k(const GLayer* __restrict__ lay, const GMember* __restrict__ mem,
                                                const GStep* __restrict__ st, GShape sh, int l, int cur) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int g = blockIdx.z, B = st[g].B;
  if (B == 0) return;
  const GLayer& ld = lay[(size_t)g * sh.L + l];
  if ((ld.K % 128 == 0) != (NB == 128)) return;
  if ((int)blockIdx.x >= ld.K / NB || (int)blockIdx.y >= 2 * pad128(B) / NB) return;
  train_nt_mask_tile<NB>(mem[g].dz[cur ^ 1], (size_t)ld.K, mem[g].dz[cur], (size_t)ld.N, ld.Wk, (size_t)ld.N, ld.N, ld.ain,
                         blockIdx.x, blockIdx.y, lds);
}

// Grid (max K / 64, max N / 64, G).
__global__ __launch_bounds__(256) void grp_adam_w_k(const GLayer* __restrict__ lay, const GStep* __restrict__ st, GShape sh, int l) {
  const int g = blockIdx.z, B = st[g].B;
  if (B == 0) return;
  const GLayer& ld = lay[(size_t)g * sh.L + l];
  if ((int)blockIdx.x >= ld.K / 64 || (int)blockIdx.y >= ld.N / 64) return;
  int slice_rows = 0;
  const int S = layer_slices(ld, sh, 2 * pad128(B), &slice_rows);
  const AdamCoef k = st[g].k;
  train_adam_w_tile(ld.Wt, ld.Wk, ld.mW, ld.vW, ld.planes, (size_t)ld.N * ld.K, S, ld.K, ld.N, k, blockIdx.x, blockIdx.y);
}

// Grid (max N / 256 rounded up, G).
__global__ void grp_adam_b_k(const GLayer* __restrict__ lay, const GStep* __restrict__ st, GShape sh, int l) {
  const int g = blockIdx.y, B = st[g].B;
  if (B == 0) return;
  const GLayer& ld = lay[(size_t)g * sh.L + l];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const AdamCoef k = st[g].k;
  if (i < ld.N) ld.b[i] = adam_entry(plane_sum(ld.bplanes, (size_t)ld.N, 2 * pad128(B) / 128, (size_t)i), ld.mb + i, ld.vb + i, ld.b[i], k);
}

__global__ void grp_cvt_k(float* __restrict__ d, const double* __restrict__ s, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n; i += (size_t)gridDim.x * blockDim.x) d[i] = (float)s[i];
}

struct Member {                                             // host side of one network
  std::vector<int> dims, kpad, npad, max_slices;
  std::vector<GLayer> lay;                                  // device pointers, as in the device table
  GMember mem{};
  float *param = nullptr, *snap = nullptr;                  // per layer Wt, Wk, b back to back; the snapshot in the same layout
  size_t param_floats = 0;
  int maxw = 0;
  long t = 0;                                               // Adam steps taken
};

}  // namespace

struct nnmpc_train_group {
  int device = 0, G = 0, L = 0;
  int nx = 0, nu = 0, with_uprev = 0, force_slices = 0, num_cus = 0;
  int max_batch = 0, cap_batch = 0;                         // the caller's limit; rounded up to 128: the workspaces
  double lr = 0, beta1 = 0, beta2 = 0, eps = 0;
  std::vector<Member> m;
  char* arena = nullptr;                                    // every per-member buffer
  GLayer* dlay = nullptr; GMember* dmem = nullptr;          // the device tables
  double* dacc = nullptr;                                   // acc of every member, contiguous: one read per call
  int n = 0;                                                // dataset rows
  float *dx = nullptr, *dup = nullptr, *dxs = nullptr, *dus = nullptr, *du = nullptr;
  char* dcall = nullptr; size_t dcall_cap = 0;              // the call's GStep table, then its row lists
  char* stage[2] = {nullptr, nullptr};                      // pinned images of it, used in turn
  hipEvent_t stage_done[2] = {nullptr, nullptr};
  size_t stage_cap[2] = {0, 0}; int stage_turn = 0;
  hipStream_t stream = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  std::vector<hipEvent_t> ev;                               // 4 per step of the last call: forward GEMMs, backward
  size_t nsets = 0;
  int64_t launches = 0;                                     // kernels enqueued by the last epoch / eval
};

namespace {
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { set_error("%s: %s", #x, hipGetErrorString(e_)); return NNMPC_EHIP; } } while (0)
#define GUARD_BEGIN try {
#define GUARD_END } catch (const std::bad_alloc&) { set_error("%s: out of host memory", __func__); return NNMPC_ENOMEM; } \
                    catch (...) { set_error("%s: unexpected exception", __func__); return NNMPC_EHIP; }

// Every kernel of a call goes through here: the count is what nnmpc_train_group_last_launches reports.
template <class... P, class... A>
void launch(nnmpc_train_group* h, void (*k)(P...), dim3 grid, dim3 block, size_t lds, A... args) {
  ++h->launches;
  hipLaunchKernelGGL(k, grid, block, lds, h->stream, args...);
}

// Lays the buffers of member g out from byte offset `off` of the arena at `base` (nullptr: sizes only); 256-byte granules.
size_t layout_member(nnmpc_train_group* h, Member& mb, char* base, size_t off) {
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return p; };
  const int L = h->L;
  const size_t Mmax = 2 * (size_t)h->cap_batch;
  mb.lay.assign(L, GLayer{});
  mb.param_floats = 0;
  for (int l = 0; l < L; ++l) mb.param_floats += 2 * (size_t)mb.npad[l] * mb.kpad[l] + mb.npad[l];   // multiples of 64 floats
  mb.param = (float*)take(mb.param_floats * 4);
  mb.snap = (float*)take(mb.param_floats * 4);
  size_t at = 0;
  std::vector<float*> act(L + 1);
  for (int l = 0; l <= L; ++l) act[l] = (float*)take(Mmax * (size_t)(l == 0 ? mb.kpad[0] : mb.npad[l - 1]) * 4);
  for (int l = 0; l < L; ++l) {
    GLayer& d = mb.lay[l];
    const size_t plane = (size_t)mb.npad[l] * mb.kpad[l], nb = mb.npad[l];
    d.K = mb.kpad[l]; d.N = mb.npad[l];
    d.Wt = mb.param ? mb.param + at : nullptr; at += plane;
    d.Wk = mb.param ? mb.param + at : nullptr; at += plane;
    d.b = mb.param ? mb.param + at : nullptr; at += nb;
    d.mW = (float*)take(plane * 4); d.vW = (float*)take(plane * 4);
    d.mb = (float*)take(nb * 4); d.vb = (float*)take(nb * 4);
    d.planes = (float*)take(plane * mb.max_slices[l] * 4);
    d.bplanes = (float*)take(nb * (Mmax / 128) * 4);
    d.ain = act[l]; d.aout = act[l + 1];
  }
  mb.mem.dz[0] = (float*)take(Mmax * mb.maxw * 4);
  mb.mem.dz[1] = (float*)take(Mmax * mb.maxw * 4);
  mb.mem.partial = (double*)take((size_t)h->cap_batch / 64 * 8);
  mb.mem.loss = (double*)take(8);
  return off;
}

// Host Keras-order weights -> the padded device images (both layouts) of layer l of a member.
int upload_layer(nnmpc_train_group* h, Member& mb, int l, const double* W, const double* b) {
  const int kp = mb.kpad[l], np_ = mb.npad[l], di = mb.dims[l], dn = mb.dims[l + 1];
  std::vector<float> wt((size_t)np_ * kp, 0.f), wk((size_t)kp * np_, 0.f), bb(np_, 0.f);
  for (int i = 0; i < di; ++i)
    for (int o = 0; o < dn; ++o) {
      const float w = (float)W[(size_t)i * dn + o];
      wt[(size_t)o * kp + i] = w; wk[(size_t)i * np_ + o] = w;
    }
  if (l < h->L - 1) for (int o = 0; o < dn; ++o) bb[o] = (float)b[o];
  HIPCHK(hipMemcpy(mb.lay[l].Wt, wt.data(), wt.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(mb.lay[l].Wk, wk.data(), wk.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(mb.lay[l].b, bb.data(), bb.size() * 4, hipMemcpyHostToDevice));
  return NNMPC_OK;
}

struct EvSet { hipEvent_t f0, f1, b0, b1; };
int ev_set(nnmpc_train_group* h, size_t i, EvSet* e) {
  while (h->ev.size() < 4 * (i + 1)) { hipEvent_t x; HIPCHK(hipEventCreate(&x)); h->ev.push_back(x); }
  *e = EvSet{h->ev[4 * i], h->ev[4 * i + 1], h->ev[4 * i + 2], h->ev[4 * i + 3]};
  return NNMPC_OK;
}

int host_pad128(int B) { return ((B + 127) / 128) * 128; }

// One lock-step step on the handle's stream: gather, forward, output, and (backward) the gradient planes and Adam, for
// the members with host[g].B > 0.  st: this step's row of the device table; rows: the device row lists, or nullptr (eval).
int enqueue_step(nnmpc_train_group* h, const GStep* host, const GStep* st, const int* rows, bool backward, size_t set) {
  const int G = h->G, L = h->L;
  const GShape sh{h->nx, h->nu, h->with_uprev, L, h->force_slices, h->num_cus};
  const GData d{h->dx, h->dup, h->dxs, h->dus, h->du};
  int Bpmax = 0;
  for (int g = 0; g < G; ++g) Bpmax = std::max(Bpmax, host_pad128(host[g].B));
  if (Bpmax == 0) return NNMPC_OK;
  const int Mmax = 2 * Bpmax;
  EvSet e;
  if (int rc = ev_set(h, set, &e)) return rc;
  struct Ext { int n = 0, k = 0, s = 0; };                  // largest extents of a tile class (0: 64, 1: 128) among the active members; 0: class absent
  launch(h, grp_gather_k, dim3(std::min(Bpmax, 2048), G), dim3(128), 0, h->dlay, st, sh, d, rows);
  hipEventRecord(e.f0, h->stream);
  for (int l = 0; l < L; ++l) {
    int nmax[2] = {0, 0};
    for (int g = 0; g < G; ++g)
      if (host[g].B) { const int N = h->m[g].npad[l]; int& x = nmax[N % 128 == 0]; x = std::max(x, N); }
    const bool last = l == L - 1;
    if (nmax[1]) {
      const dim3 grid(nmax[1] / 128, Mmax / 128, G);
      if (last) launch(h, grp_fwd_k<128, false, false>, grid, dim3(256), TileCfg<128>::LDS_FLOATS * 4, h->dlay, st, sh, l);
      else launch(h, grp_fwd_k<128, true, true>, grid, dim3(256), TileCfg<128>::LDS_FLOATS * 4, h->dlay, st, sh, l);
    }
    if (nmax[0]) {
      const dim3 grid(nmax[0] / 64, Mmax / 64, G);
      if (last) launch(h, grp_fwd_k<64, false, false>, grid, dim3(256), TileCfg<64>::LDS_FLOATS * 4, h->dlay, st, sh, l);
      else launch(h, grp_fwd_k<64, true, true>, grid, dim3(256), TileCfg<64>::LDS_FLOATS * 4, h->dlay, st, sh, l);
    }
  }
  hipEventRecord(e.f1, h->stream);
  launch(h, grp_output_k, dim3(Bpmax / 64, G), dim3(256), 0, h->dlay, h->dmem, st, sh, d, rows, backward ? 1 : 0);
  launch(h, grp_loss_finish_k, dim3(G), dim3(64), 0, h->dmem, st);
  hipEventRecord(e.b0, h->stream);
  if (backward) {
    int cur = 0;
    for (int l = L - 1; l >= 0; --l) {
      Ext dw[2], da[2];
      int nall = 0;
      for (int g = 0; g < G; ++g) {
        if (!host[g].B) continue;
        const Member& mb = h->m[g];
        const int K = mb.kpad[l], N = mb.npad[l], M = 2 * host_pad128(host[g].B);
        const int big = N % 128 == 0 && K % 128 == 0, nb = big ? 128 : 64;
        int slice_rows = 0;
        const int S = dw_slices(h->force_slices, h->num_cus, M, (N / nb) * (K / nb), &slice_rows);
        if (S > mb.max_slices[l]) { set_error("nnmpc_train_group: %d dW slices for layer %d of member %d, planes for %d", S, l, g, mb.max_slices[l]); return NNMPC_EINVAL; }
        dw[big].n = std::max(dw[big].n, N); dw[big].k = std::max(dw[big].k, K); dw[big].s = std::max(dw[big].s, S);
        Ext& a = da[K % 128 == 0];
        a.k = std::max(a.k, K);
        nall = std::max(nall, N);
      }
      if (dw[1].s) launch(h, grp_dw_k<128>, dim3(dw[1].k / 128, dw[1].n / 128, G * dw[1].s), dim3(256), TileCfgTN<128>::LDS_FLOATS * 4,
                          h->dlay, h->dmem, st, sh, l, cur, dw[1].s);
      if (dw[0].s) launch(h, grp_dw_k<64>, dim3(dw[0].k / 64, dw[0].n / 64, G * dw[0].s), dim3(256), TileCfgTN<64>::LDS_FLOATS * 4,
                          h->dlay, h->dmem, st, sh, l, cur, dw[0].s);
      if (l < L - 1) launch(h, grp_colsum_k, dim3(nall / 64, Mmax / 128, G), dim3(256), 0, h->dlay, h->dmem, st, sh, l, cur);
      if (l > 0) {
        if (da[1].k) launch(h, grp_da_k<128>, dim3(da[1].k / 128, Mmax / 128, G), dim3(256), TileCfg<128>::LDS_FLOATS * 4,
                            h->dlay, h->dmem, st, sh, l, cur);
        if (da[0].k) launch(h, grp_da_k<64>, dim3(da[0].k / 64, Mmax / 64, G), dim3(256), TileCfg<64>::LDS_FLOATS * 4,
                            h->dlay, h->dmem, st, sh, l, cur);
        cur ^= 1;
      }
    }
  }
  hipEventRecord(e.b1, h->stream);
  if (backward)
    for (int l = 0; l < L; ++l) {
      int nall = 0, kall = 0;
      for (int g = 0; g < G; ++g)
        if (host[g].B) { nall = std::max(nall, h->m[g].npad[l]); kall = std::max(kall, h->m[g].kpad[l]); }
      launch(h, grp_adam_w_k, dim3(kall / 64, nall / 64, G), dim3(256), 0, h->dlay, st, sh, l);
      if (l < L - 1) launch(h, grp_adam_b_k, dim3((nall + 255) / 256, G), dim3(256), 0, h->dlay, st, sh, l);
    }
  return NNMPC_OK;
}

// The call's GStep table (steps x G) and, behind it, its row lists go to the device in ONE copy out of a pinned image.
// Two images are used in turn; before one is overwritten the host waits for the upload that last read it.
int upload_call(nnmpc_train_group* h, const std::vector<GStep>& tab, const int32_t* rows, size_t nrows) {
  const size_t tb = tab.size() * sizeof(GStep), bytes = tb + nrows * 4;
  if (bytes > h->dcall_cap) {
    HIPCHK(stream_sync(h->stream));
    if (h->dcall) { hipFree(h->dcall); h->dcall = nullptr; h->dcall_cap = 0; }
    void* q = nullptr;
    if (hipMalloc(&q, bytes) != hipSuccess) { set_error("hipMalloc(%zu) failed", bytes); return NNMPC_ENOMEM; }
    h->dcall = (char*)q; h->dcall_cap = bytes;
  }
  const int k = h->stage_turn;
  h->stage_turn ^= 1;
  if (!h->stage_done[k]) HIPCHK(hipEventCreateWithFlags(&h->stage_done[k], hipEventDisableTiming));
  else HIPCHK(hipEventSynchronize(h->stage_done[k]));
  if (bytes > h->stage_cap[k]) {
    if (h->stage[k]) { hipHostFree(h->stage[k]); h->stage[k] = nullptr; h->stage_cap[k] = 0; }
    void* q = nullptr;
    if (hipHostMalloc(&q, bytes, hipHostMallocDefault) != hipSuccess) { set_error("hipHostMalloc(%zu) failed", bytes); return NNMPC_ENOMEM; }
    h->stage[k] = (char*)q; h->stage_cap[k] = bytes;
  }
  memcpy(h->stage[k], tab.data(), tb);
  if (nrows) memcpy(h->stage[k] + tb, rows, nrows * 4);
  HIPCHK(hipMemcpyAsync(h->dcall, h->stage[k], bytes, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipEventRecord(h->stage_done[k], h->stream));
  return NNMPC_OK;
}

int read_acc(nnmpc_train_group* h, std::vector<double>& out) {
  out.assign(h->G, 0.0);
  HIPCHK(hipMemcpyAsync(out.data(), h->dacc, (size_t)h->G * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(stream_sync(h->stream));
  HIPCHK(hipGetLastError());
  return NNMPC_OK;
}

int check_member(const nnmpc_train_group* h, const char* who, int g) {
  if (g < 0 || g >= h->G) { set_error("%s: member %d of a group of %d", who, g, h->G); return NNMPC_EINVAL; }
  return NNMPC_OK;
}
}  // namespace

extern "C" {

int nnmpc_train_group_destroy(nnmpc_train_group* h) {
  if (!h) return NNMPC_OK;
  hipSetDevice(h->device);
  hipDeviceSynchronize();
  for (void* p : {(void*)h->arena, (void*)h->dlay, (void*)h->dmem, (void*)h->dacc, (void*)h->dcall, (void*)h->dx, (void*)h->dup,
                  (void*)h->dxs, (void*)h->dus, (void*)h->du})
    if (p) hipFree(p);
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

int nnmpc_train_group_create(nnmpc_train_group** out, int32_t G, int32_t nlayers, const int32_t* dims, const double* const* W,
                             const double* const* b, int32_t nx, int32_t nu, int32_t with_uprev, int32_t max_batch,
                             double lr, double beta1, double beta2, double eps) {
  GUARD_BEGIN
  if (!out || nlayers < 1 || !dims || !W || !b || nx <= 0 || nu <= 0 || max_batch < 1) { set_error("nnmpc_train_group_create: bad arguments"); return NNMPC_EINVAL; }
  if (G < 1) { set_error("nnmpc_train_group_create: a group of %d networks", G); return NNMPC_EINVAL; }
  const int din = 2 * nx + (with_uprev ? 2 : 1) * nu, L = nlayers;
  for (int g = 0; g < G; ++g) {
    const int32_t* dg = dims + (size_t)g * (L + 1);
    if (dg[0] != din || dg[L] != nu) { set_error("nnmpc_train_group_create: member %d: dims[0]=%d (want %d), dims[L]=%d (want %d)", g, dg[0], din, dg[L], nu); return NNMPC_EINVAL; }
    for (int l = 0; l <= L; ++l)
      if (dg[l] < 1) { set_error("nnmpc_train_group_create: member %d: dims[%d]=%d", g, l, dg[l]); return NNMPC_EINVAL; }
    for (int l = 0; l < L; ++l)
      if (!W[(size_t)g * L + l] || (l < L - 1 && !b[(size_t)g * L + l])) { set_error("nnmpc_train_group_create: member %d: missing weights or bias of layer %d", g, l); return NNMPC_EINVAL; }
  }
  if (!(lr > 0) || !(beta1 >= 0 && beta1 < 1) || !(beta2 >= 0 && beta2 < 1) || !(eps > 0)) { set_error("nnmpc_train_group_create: bad Adam parameters (lr > 0, 0 <= beta < 1, eps > 0: with eps = 0 an entry whose gradient is exactly zero, all padding included, would become 0 / 0)"); return NNMPC_EINVAL; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { set_error("nnmpc_train_group_create: no HIP device available (no CPU fallback)"); return NNMPC_EHIP; }
  struct Destroy { void operator()(nnmpc_train_group* p) const { nnmpc_train_group_destroy(p); } };
  std::unique_ptr<nnmpc_train_group, Destroy> guard(new nnmpc_train_group());
  nnmpc_train_group* h = guard.get();
  HIPCHK(hipGetDevice(&h->device));
  HIPCHK(hipDeviceGetAttribute(&h->num_cus, hipDeviceAttributeMultiprocessorCount, h->device));
  if (h->num_cus < 1) { set_error("nnmpc_train_group_create: device reports %d compute units", h->num_cus); return NNMPC_EHIP; }
  h->G = G; h->L = L; h->nx = nx; h->nu = nu; h->with_uprev = with_uprev != 0;
  h->max_batch = max_batch;
  h->cap_batch = ((max_batch + 127) / 128) * 128;
  h->lr = lr; h->beta1 = beta1; h->beta2 = beta2; h->eps = eps;
  if (const char* e = getenv("NNMPC_TRAIN_DW_SLICES")) h->force_slices = std::max(0, atoi(e));   // tests: several slices on a small batch
  if (hipStreamCreate(&h->stream) != hipSuccess || hipEventCreate(&h->e0) != hipSuccess || hipEventCreate(&h->e1) != hipSuccess) {
    set_error("nnmpc_train_group_create: stream / event creation failed"); return NNMPC_EHIP;
  }
  HIPCHK(hipFuncSetAttribute((const void*)grp_fwd_k<128, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, TileCfg<128>::LDS_FLOATS * 4));
  HIPCHK(hipFuncSetAttribute((const void*)grp_fwd_k<128, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, TileCfg<128>::LDS_FLOATS * 4));
  HIPCHK(hipFuncSetAttribute((const void*)grp_da_k<128>, hipFuncAttributeMaxDynamicSharedMemorySize, TileCfg<128>::LDS_FLOATS * 4));
  HIPCHK(hipFuncSetAttribute((const void*)grp_dw_k<128>, hipFuncAttributeMaxDynamicSharedMemorySize, TileCfgTN<128>::LDS_FLOATS * 4));
  const int Mmax = 2 * h->cap_batch;
  h->m.resize(G);
  size_t bytes = 0;
  for (int g = 0; g < G; ++g) {
    Member& mb = h->m[g];
    const int32_t* dg = dims + (size_t)g * (L + 1);
    mb.dims.assign(dg, dg + L + 1);
    for (int l = 0; l < L; ++l) {
      const int kp = l == 0 ? ((dg[0] + 63) / 64) * 64 : mb.npad[l - 1];
      const int np_ = dg[l + 1] > 64 ? ((dg[l + 1] + 127) / 128) * 128 : 64;   // as nnmpc_nn_create
      mb.kpad.push_back(kp); mb.npad.push_back(np_);
      mb.maxw = std::max(mb.maxw, std::max(kp, np_));
      const int nb = (np_ % 128 == 0 && kp % 128 == 0) ? 128 : 64;
      mb.max_slices.push_back(dw_slices_wanted(h->force_slices, h->num_cus, Mmax, (np_ / nb) * (kp / nb)));
    }
    bytes = layout_member(h, mb, nullptr, bytes);
    for (int S : mb.max_slices)                             // the dW grid carries member x slice in z
      if ((int64_t)G * S > 65535) { set_error("nnmpc_train_group_create: %d members x %d dW slices exceed a grid's z extent", G, S); return NNMPC_EINVAL; }
  }
  void* q = nullptr;
  if (hipMalloc(&q, bytes) != hipSuccess) { set_error("nnmpc_train_group_create: hipMalloc(%zu) failed", bytes); return NNMPC_ENOMEM; }
  h->arena = (char*)q;
  HIPCHK(hipMemset(h->arena, 0, bytes));
  if (hipMalloc(&q, (size_t)G * 8) != hipSuccess) { set_error("nnmpc_train_group_create: hipMalloc failed"); return NNMPC_ENOMEM; }
  h->dacc = (double*)q;
  HIPCHK(hipMemset(h->dacc, 0, (size_t)G * 8));
  std::vector<GLayer> lay;
  std::vector<GMember> mem;
  size_t off = 0;
  for (int g = 0; g < G; ++g) {
    Member& mb = h->m[g];
    off = layout_member(h, mb, h->arena, off);
    mb.mem.acc = h->dacc + g;
    for (int l = 0; l < L; ++l)
      if (int rc = upload_layer(h, mb, l, W[(size_t)g * L + l], b[(size_t)g * L + l])) return rc;
    HIPCHK(hipMemcpy(mb.snap, mb.param, mb.param_floats * 4, hipMemcpyDeviceToDevice));   // the snapshot starts as the initial weights
    lay.insert(lay.end(), mb.lay.begin(), mb.lay.end());
    mem.push_back(mb.mem);
  }
  if (hipMalloc(&q, lay.size() * sizeof(GLayer)) != hipSuccess) { set_error("nnmpc_train_group_create: hipMalloc failed"); return NNMPC_ENOMEM; }
  h->dlay = (GLayer*)q;
  if (hipMalloc(&q, mem.size() * sizeof(GMember)) != hipSuccess) { set_error("nnmpc_train_group_create: hipMalloc failed"); return NNMPC_ENOMEM; }
  h->dmem = (GMember*)q;
  HIPCHK(hipMemcpy(h->dlay, lay.data(), lay.size() * sizeof(GLayer), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->dmem, mem.data(), mem.size() * sizeof(GMember), hipMemcpyHostToDevice));
  *out = guard.release();
  return NNMPC_OK;
  GUARD_END
}

int nnmpc_train_group_set_data(nnmpc_train_group* h, int32_t n, const double* x, const double* uprev, const double* xs,
                               const double* us, const double* u, int32_t ptr_kind) {
  GUARD_BEGIN
  if (!h || n < 1 || !x || !xs || !us || !u) { set_error("nnmpc_train_group_set_data: bad arguments"); return NNMPC_EINVAL; }
  if (h->with_uprev && !uprev) { set_error("nnmpc_train_group_set_data: the networks take uprev, none given"); return NNMPC_EINVAL; }
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(stream_sync(h->stream));
  for (float** p : {&h->dx, &h->dup, &h->dxs, &h->dus, &h->du}) { if (*p) hipFree(*p); *p = nullptr; }
  h->n = 0;
  struct { float** d; const double* s; int w; } col[5] = {{&h->dx, x, h->nx}, {&h->dup, h->with_uprev ? uprev : nullptr, h->nu},
                                                          {&h->dxs, xs, h->nx}, {&h->dus, us, h->nu}, {&h->du, u, h->nu}};
  std::vector<float> tmp;
  for (auto& c : col) {
    if (!c.s) continue;
    const size_t cnt = (size_t)n * c.w;
    void* q = nullptr;
    if (hipMalloc(&q, cnt * 4) != hipSuccess) { set_error("hipMalloc(%zu) failed", cnt * 4); return NNMPC_ENOMEM; }
    *c.d = (float*)q;
    if (ptr_kind == NNMPC_HOST) {
      tmp.resize(cnt);
      for (size_t i = 0; i < cnt; ++i) tmp[i] = (float)c.s[i];
      HIPCHK(hipMemcpy(*c.d, tmp.data(), cnt * 4, hipMemcpyHostToDevice));
    } else {
      hipLaunchKernelGGL(grp_cvt_k, dim3(1024), dim3(256), 0, h->stream, *c.d, c.s, cnt);
    }
  }
  HIPCHK(stream_sync(h->stream));
  HIPCHK(hipGetLastError());
  h->n = n;
  return NNMPC_OK;
  GUARD_END
}

int nnmpc_train_group_epoch(nnmpc_train_group* h, const int32_t* nrows, const int32_t* perm, int32_t batch, double* loss) {
  GUARD_BEGIN
  if (!h || !nrows || !perm) { set_error("nnmpc_train_group_epoch: bad arguments"); return NNMPC_EINVAL; }
  if (!h->dx) { set_error("nnmpc_train_group_epoch: no dataset (call nnmpc_train_group_set_data first)"); return NNMPC_EINVAL; }
  if (batch < 1 || batch > h->max_batch) { set_error("nnmpc_train_group_epoch: batch of %d rows, max_batch is %d", batch, h->max_batch); return NNMPC_EINVAL; }
  const int G = h->G;
  size_t total = 0;
  int steps = 0;
  for (int g = 0; g < G; ++g) {
    if (nrows[g] < 0) { set_error("nnmpc_train_group_epoch: member %d: %d rows", g, nrows[g]); return NNMPC_EINVAL; }
    total += (size_t)nrows[g];
    steps = std::max(steps, (nrows[g] + batch - 1) / batch);
  }
  if (total > (size_t)INT32_MAX) { set_error("nnmpc_train_group_epoch: %zu rows in all, at most 2^31 - 1", total); return NNMPC_EINVAL; }
  for (size_t i = 0; i < total; ++i)
    if (perm[i] < 0 || perm[i] >= h->n) { set_error("nnmpc_train_group_epoch: row index %d at position %zu outside [0, %d)", perm[i], i, h->n); return NNMPC_EINVAL; }
  if (loss) for (int g = 0; g < G; ++g) loss[g] = NAN;      // a member without rows has no loss
  h->launches = 0; h->nsets = 0;
  if (steps == 0) return NNMPC_OK;
  HIPCHK(hipSetDevice(h->device));
  // the table: per member the batches of nnmpc_train_epoch (the last one is the short one), each with the scalars of its own Adam step
  std::vector<GStep> tab((size_t)steps * G, GStep{});
  size_t at = 0;
  for (int g = 0; g < G; ++g) {
    for (int i = 0, k = 0; i < nrows[g]; i += batch, ++k) {
      GStep& s = tab[(size_t)k * G + g];
      const int B = std::min(batch, nrows[g] - i);
      s.k = adam_coef(h->lr, h->beta1, h->beta2, h->eps, h->m[g].t + k + 1);
      s.loss_scale = 1.0 / ((double)B * h->nu); s.acc_w = (double)B;
      s.gscale = (float)(2.0 / ((double)B * h->nu));
      s.B = B; s.at = (int)(at + i);
    }
    at += nrows[g];
  }
  if (int rc = upload_call(h, tab, perm, total)) return rc;
  const GStep* dtab = (const GStep*)h->dcall;
  const int* drows = (const int*)(h->dcall + tab.size() * sizeof(GStep));
  hipStream_t s = h->stream;
  HIPCHK(hipMemsetAsync(h->dacc, 0, (size_t)G * 8, s));
  hipEventRecord(h->e0, s);
  for (int k = 0; k < steps; ++k)
    if (int rc = enqueue_step(h, &tab[(size_t)k * G], dtab + (size_t)k * G, drows, true, k)) return rc;
  for (int g = 0; g < G; ++g) h->m[g].t += (nrows[g] + batch - 1) / batch;
  h->nsets = steps;
  hipEventRecord(h->e1, s);
  std::vector<double> sum;
  if (int rc = read_acc(h, sum)) return rc;
  if (loss) for (int g = 0; g < G; ++g) if (nrows[g]) loss[g] = sum[g] / (double)nrows[g];
  return NNMPC_OK;
  GUARD_END
}

int nnmpc_train_group_eval(nnmpc_train_group* h, const int32_t* first, const int32_t* count, double* mse) {
  GUARD_BEGIN
  if (!h || !first || !count || !mse) { set_error("nnmpc_train_group_eval: bad arguments"); return NNMPC_EINVAL; }
  if (!h->dx) { set_error("nnmpc_train_group_eval: no dataset (call nnmpc_train_group_set_data first)"); return NNMPC_EINVAL; }
  const int G = h->G;
  int steps = 0;
  for (int g = 0; g < G; ++g) {
    if (count[g] < 0 || (count[g] > 0 && (first[g] < 0 || (int64_t)first[g] + count[g] > h->n))) {
      set_error("nnmpc_train_group_eval: member %d: rows [%d, %d + %d) outside [0, %d)", g, first[g], first[g], count[g], h->n); return NNMPC_EINVAL;
    }
    steps = std::max(steps, (count[g] + h->max_batch - 1) / h->max_batch);
  }
  for (int g = 0; g < G; ++g) mse[g] = NAN;                 // a member without rows has no loss
  h->launches = 0; h->nsets = 0;
  if (steps == 0) return NNMPC_OK;
  HIPCHK(hipSetDevice(h->device));
  std::vector<GStep> tab((size_t)steps * G, GStep{});
  for (int g = 0; g < G; ++g)
    for (int i = 0, k = 0; i < count[g]; i += h->max_batch, ++k) {
      GStep& s = tab[(size_t)k * G + g];
      const int B = std::min(h->max_batch, count[g] - i);
      s.loss_scale = 1.0; s.acc_w = 1.0;
      s.gscale = (float)(2.0 / ((double)B * h->nu));
      s.B = B; s.at = first[g] + i;
    }
  if (int rc = upload_call(h, tab, nullptr, 0)) return rc;
  const GStep* dtab = (const GStep*)h->dcall;
  hipStream_t s = h->stream;
  HIPCHK(hipMemsetAsync(h->dacc, 0, (size_t)G * 8, s));
  hipEventRecord(h->e0, s);
  for (int k = 0; k < steps; ++k)
    if (int rc = enqueue_step(h, &tab[(size_t)k * G], dtab + (size_t)k * G, nullptr, false, k)) return rc;
  h->nsets = steps;
  hipEventRecord(h->e1, s);
  std::vector<double> sum;
  if (int rc = read_acc(h, sum)) return rc;
  for (int g = 0; g < G; ++g) if (count[g]) mse[g] = sum[g] / ((double)count[g] * h->nu);
  return NNMPC_OK;
  GUARD_END
}

int nnmpc_train_group_get_weights(nnmpc_train_group* h, int32_t g, double* const* W, double* const* b) {
  GUARD_BEGIN
  if (!h || !W || !b) { set_error("nnmpc_train_group_get_weights: bad arguments"); return NNMPC_EINVAL; }
  if (int rc = check_member(h, "nnmpc_train_group_get_weights", g)) return rc;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(stream_sync(h->stream));
  const Member& mb = h->m[g];
  std::vector<float> tmp;
  for (int l = 0; l < h->L; ++l) {
    const int kp = mb.kpad[l], np_ = mb.npad[l], di = mb.dims[l], dn = mb.dims[l + 1];
    if (W[l]) {
      tmp.resize((size_t)np_ * kp);
      HIPCHK(hipMemcpy(tmp.data(), mb.lay[l].Wt, tmp.size() * 4, hipMemcpyDeviceToHost));
      for (int i = 0; i < di; ++i)
        for (int o = 0; o < dn; ++o) W[l][(size_t)i * dn + o] = (double)tmp[(size_t)o * kp + i];
    }
    if (l < h->L - 1 && b[l]) {
      tmp.resize(np_);
      HIPCHK(hipMemcpy(tmp.data(), mb.lay[l].b, (size_t)np_ * 4, hipMemcpyDeviceToHost));
      for (int o = 0; o < dn; ++o) b[l][o] = (double)tmp[o];
    }
  }
  return NNMPC_OK;
  GUARD_END
}

int nnmpc_train_group_set_weights(nnmpc_train_group* h, int32_t g, const double* const* W, const double* const* b) {
  GUARD_BEGIN
  if (!h || !W || !b) { set_error("nnmpc_train_group_set_weights: bad arguments"); return NNMPC_EINVAL; }
  if (int rc = check_member(h, "nnmpc_train_group_set_weights", g)) return rc;
  for (int l = 0; l < h->L; ++l)
    if (!W[l] || (l < h->L - 1 && !b[l])) { set_error("nnmpc_train_group_set_weights: missing weights or bias of layer %d", l); return NNMPC_EINVAL; }
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(stream_sync(h->stream));
  for (int l = 0; l < h->L; ++l)
    if (int rc = upload_layer(h, h->m[g], l, W[l], b[l])) return rc;
  return NNMPC_OK;
  GUARD_END
}

// One device-side copy per chosen member: its weights of every layer lie back to back, the snapshot in the same layout.
static int copy_params(nnmpc_train_group* h, const char* who, const int32_t* mask, bool to_snapshot) {
  if (!h || !mask) { set_error("%s: bad arguments", who); return NNMPC_EINVAL; }
  HIPCHK(hipSetDevice(h->device));
  for (int g = 0; g < h->G; ++g) {
    if (!mask[g]) continue;
    Member& mb = h->m[g];
    HIPCHK(hipMemcpyAsync(to_snapshot ? mb.snap : mb.param, to_snapshot ? mb.param : mb.snap, mb.param_floats * 4,
                          hipMemcpyDeviceToDevice, h->stream));
  }
  return NNMPC_OK;
}

int nnmpc_train_group_snapshot(nnmpc_train_group* h, const int32_t* mask) {
  return copy_params(h, "nnmpc_train_group_snapshot", mask, true);
}

int nnmpc_train_group_restore(nnmpc_train_group* h, const int32_t* mask) {
  return copy_params(h, "nnmpc_train_group_restore", mask, false);
}

int nnmpc_train_group_last_ms(nnmpc_train_group* h, double* gemm_ms, double* total_ms) {
  if (!h) { set_error("nnmpc_train_group_last_ms: bad arguments"); return NNMPC_EINVAL; }
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

int nnmpc_train_group_last_launches(nnmpc_train_group* h, int64_t* n) {
  if (!h || !n) { set_error("nnmpc_train_group_last_launches: bad arguments"); return NNMPC_EINVAL; }
  *n = h->launches;
  return NNMPC_OK;
}

int nnmpc_train_group_padding_max(nnmpc_train_group* h, double* maxabs) {
  GUARD_BEGIN
  if (!h || !maxabs) { set_error("nnmpc_train_group_padding_max: bad arguments"); return NNMPC_EINVAL; }
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(stream_sync(h->stream));
  double mx = 0.0;
  std::vector<float> tmp;
  auto fold = [&](float v) { const double a = fabs((double)v); if (mx == mx && !(a <= mx)) mx = a; };   // a NaN in the padding counts, and stays
  for (const Member& mb : h->m)
    for (int l = 0; l < h->L; ++l) {
      const int kp = mb.kpad[l], np_ = mb.npad[l], di = mb.dims[l], dn = mb.dims[l + 1];
      const GLayer& d = mb.lay[l];
      tmp.resize((size_t)np_ * kp);
      for (float* p : {d.Wt, d.mW, d.vW}) {                   // [out][in]
        HIPCHK(hipMemcpy(tmp.data(), p, tmp.size() * 4, hipMemcpyDeviceToHost));
        for (int o = 0; o < np_; ++o)
          for (int i = 0; i < kp; ++i) if (o >= dn || i >= di) fold(tmp[(size_t)o * kp + i]);
      }
      HIPCHK(hipMemcpy(tmp.data(), d.Wk, tmp.size() * 4, hipMemcpyDeviceToHost));   // [in][out]
      for (int i = 0; i < kp; ++i)
        for (int o = 0; o < np_; ++o) if (o >= dn || i >= di) fold(tmp[(size_t)i * np_ + o]);
      for (float* p : {d.b, d.mb, d.vb}) {
        HIPCHK(hipMemcpy(tmp.data(), p, (size_t)np_ * 4, hipMemcpyDeviceToHost));
        for (int o = (l < h->L - 1 ? dn : 0); o < np_; ++o) fold(tmp[o]);
      }
    }
  *maxabs = mx;
  return NNMPC_OK;
  GUARD_END
}

}  // extern "C"
