// Host side of the training step, once, for nn_train.hip (one network per handle) and nn_train_group.hip (a sweep of
// networks per launch): what a handle of either kind holds besides its networks (TrainCommon), how one network lies in
// device memory (Member, GLayer, GMember), and the functions over the two -- the padding and slice rule, layout, weight
// upload and read-back, the padding scan, the dataset, event sets, the staged upload, snapshot / restore, and the argument
// checks.  The two files keep their own kernels and enqueue order; everything else about a network is here, so a member
// of a group and a single handle are laid out, padded, sliced, uploaded and read back by the same code.
// `who` is the ABI function the caller called: every message starts with it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <math.h>
#include <vector>
#include <algorithm>
#include "nn_train_dev.h"
#include "dev_res.h"

namespace nnmpc {
namespace {

struct GLayer {                                             // operands of layer l of a network
  float *Wt, *Wk, *b, *mW, *vW, *mb, *vb;                   // Wt [N][K], Wk [K][N]
  float *planes, *bplanes;                                  // dW / db partial planes
  float *ain, *aout;                                        // activations [train_rows(form, cap_batch)][K], [..][N]
  int K, N;                                                 // padded input / output width
};
struct GMember { float* dz[2]; double *partial, *loss, *acc; };   // acc: the owner of the handle places it

struct Member {                                             // host side of one network
  std::vector<int> dims, kpad, npad, max_slices;
  std::vector<GLayer> lay;                                  // device pointers
  GMember mem{};
  float *param = nullptr, *snap = nullptr;                  // per layer Wt, Wk, b back to back; the snapshot in the same layout
  size_t param_floats = 0;
  int maxw = 0;
  long t = 0;                                               // Adam steps taken
};

struct TrainCommon {                                        // what a handle holds besides its networks
  int device = 0, L = 0;
  int nx = 0, nu = 0, with_uprev = 0, force_slices = 0, num_cus = 0;
  int form = NNMPC_NN_STRUCTURED;                           // NNMPC_NN_*: two stacked passes and a bias-free head, or one pass and a head bias (with a ReLU: _RELU)
  int max_batch = 0, cap_batch = 0;                         // the caller's limit (what B is checked against); rounded up to 128: the workspaces
  double lr = 0, beta1 = 0, beta2 = 0, eps = 0;
  int n = 0;                                                // dataset rows
  float *dx = nullptr, *dup = nullptr, *dxs = nullptr, *dus = nullptr, *du = nullptr;
  // The tangent loss (nnmpc_train_create_tan, nnmpc_train_create_group_tan): the handle stacks a third row block, tdx / tdup /
  // tt are the dataset's directions and targets as f32.  tan_w is a single handle's weight w of the tangent term (0: the
  // plain step); a group keeps one weight per member itself and leaves tan_w alone.
  // nnmpc_train_create_tan_ex: tan_dirs directions per row ([n][D][.] columns, D tangent blocks) and, tan_whole, directions
  // over the whole network input: tdxs / tdus are their xs and us parts and pass 2 gets D tangent blocks of its own.
  int tan = 0, tan_dirs = 1, tan_whole = 0;
  double tan_w = 0.0;
  float *tdx = nullptr, *tdup = nullptr, *tdxs = nullptr, *tdus = nullptr, *tt = nullptr;
  char* dcall = nullptr;                                    // what the last call uploaded: its row lists (behind its step table, in a group)
  hipEvent_t stage_done[2] = {nullptr, nullptr};            // the upload out of the pinned image k (used in turn) has finished
  int stage_turn = 0;
  hipStream_t stream = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  size_t nsets = 0;
  // Owns all of it and the networks' buffers.  Slot 0: dcall; pinned slots 0, 1: its two images; pool: 4 events per step of
  // the last call (around the forward GEMMs, around the backward).
  DevRes res{1, 2};
};

inline int pad128_host(int B) { return ((B + 127) / 128) * 128; }
// Most stacked rows of a batch of Bp padded samples on this handle: what its workspaces and planes are sized for.
inline int max_rows(const TrainCommon& c, int Bp) { return train_rows_tan(c.form, Bp, c.tan, c.tan_dirs, c.tan_whole); }
// The tangent term is part of this handle's loss.
inline bool tan_active(const TrainCommon& c) { return c.tan && c.tan_w > 0.0; }

// ---- argument checks that need no device (made before one is looked for) ----

inline int check_form(const char* who, int form) {
  if (form != NNMPC_NN_STRUCTURED && form != NNMPC_NN_UNSTD && form != NNMPC_NN_UNSTD_RELU) { set_error("%s: form %d (NNMPC_NN_STRUCTURED, NNMPC_NN_UNSTD or NNMPC_NN_UNSTD_RELU)", who, form); return NNMPC_EINVAL; }
  return NNMPC_OK;
}
inline bool has_bias(int form, int L, int l) { return l < L - 1 || form != NNMPC_NN_STRUCTURED; }   // the head has one in the unstructured forms
// One network's dims, W, b against nx, nu and the form; `mem`: what a group puts in front ("member 2: "), or "".
inline int check_network(const char* who, const char* mem, int L, const int32_t* dims, const double* const* W,
                         const double* const* b, int nx, int nu, int with_uprev, int form) {
  const int din = 2 * nx + (with_uprev ? 2 : 1) * nu;
  if (dims[0] != din || dims[L] != nu) { set_error("%s: %sdims[0]=%d (want %d), dims[L]=%d (want %d)", who, mem, dims[0], din, dims[L], nu); return NNMPC_EINVAL; }
  for (int l = 0; l <= L; ++l)
    if (dims[l] < 1) { set_error("%s: %sdims[%d]=%d", who, mem, l, dims[l]); return NNMPC_EINVAL; }
  for (int l = 0; l < L; ++l)
    if (!W[l] || (has_bias(form, L, l) && !b[l])) { set_error("%s: %smissing weights or bias of layer %d", who, mem, l); return NNMPC_EINVAL; }
  return NNMPC_OK;
}
inline int check_adam(const char* who, double lr, double beta1, double beta2, double eps) {
  if (!(lr > 0) || !(beta1 >= 0 && beta1 < 1) || !(beta2 >= 0 && beta2 < 1) || !(eps > 0)) { set_error("%s: bad Adam parameters (lr > 0, 0 <= beta < 1, eps > 0: with eps = 0 an entry whose gradient is exactly zero, all padding included, would become 0 / 0)", who); return NNMPC_EINVAL; }
  return NNMPC_OK;
}
inline int check_data(const TrainCommon& c, const char* who) {
  if (!c.dx) { set_error("%s: no dataset (set_data comes first)", who); return NNMPC_EINVAL; }
  return NNMPC_OK;
}
inline int check_batch(const TrainCommon& c, const char* who, int B) {   // and that there are rows to take it from
  if (int rc = check_data(c, who)) return rc;
  if (B < 1 || B > c.max_batch) { set_error("%s: batch of %d rows, max_batch is %d", who, B, c.max_batch); return NNMPC_EINVAL; }
  return NNMPC_OK;
}
inline int check_rows(const TrainCommon& c, const char* who, size_t count, const int32_t* rows) {
  for (size_t i = 0; i < count; ++i)
    if (rows[i] < 0 || rows[i] >= c.n) { set_error("%s: row index %d at position %zu outside [0, %d)", who, rows[i], i, c.n); return NNMPC_EINVAL; }
  return NNMPC_OK;
}

// ---- the handle's common part ----

// Device, compute units, the slice override (read once, here), stream and the call's two events.
inline int common_init(const char* who, TrainCommon& c, int L, int nx, int nu, int with_uprev, int max_batch, double lr,
                       double beta1, double beta2, double eps, int form) {
  HIPCHK(hipGetDevice(&c.device));
  c.res.device = c.device;
  HIPCHK(hipDeviceGetAttribute(&c.num_cus, hipDeviceAttributeMultiprocessorCount, c.device));
  if (c.num_cus < 1) { set_error("%s: device reports %d compute units", who, c.num_cus); return NNMPC_EHIP; }
  c.L = L; c.nx = nx; c.nu = nu; c.with_uprev = with_uprev != 0; c.form = form;
  c.max_batch = max_batch;
  c.cap_batch = pad128_host(max_batch);
  c.lr = lr; c.beta1 = beta1; c.beta2 = beta2; c.eps = eps;
  if (const char* e = getenv("NNMPC_TRAIN_DW_SLICES")) c.force_slices = std::max(0, atoi(e));   // tests: several slices on a small batch
  if (int rc = c.res.stream(&c.stream)) return rc;
  if (int rc = c.res.event(&c.e0)) return rc;
  return c.res.event(&c.e1);
}

// ---- one network ----

// The padding rule (as nnmpc_nn_create: input to 64, wide layers to 128, head to 64) and the most dW slices a layer can
// take (dw_slices_wanted is non-decreasing in M: its value at the most stacked rows, max_rows(c, cap_batch), sizes the planes).
inline void member_shapes(const TrainCommon& c, Member& mb, const int32_t* dims) {
  mb.dims.assign(dims, dims + c.L + 1);
  for (int l = 0; l < c.L; ++l) {
    const int kp = l == 0 ? ((dims[0] + 63) / 64) * 64 : mb.npad[l - 1];
    const int np_ = dims[l + 1] > 64 ? ((dims[l + 1] + 127) / 128) * 128 : 64;
    mb.kpad.push_back(kp); mb.npad.push_back(np_);
    mb.maxw = std::max(mb.maxw, std::max(kp, np_));
    const int nb = (np_ % 128 == 0 && kp % 128 == 0) ? 128 : 64;
    mb.max_slices.push_back(dw_slices_wanted(c.force_slices, c.num_cus, max_rows(c, c.cap_batch), (np_ / nb) * (kp / nb)));
  }
}
// The dW slices of layer l at M stacked rows and their row count: the rule of nn_train_dev.h at this handle's device and override.
inline int member_slices(const TrainCommon& c, const Member& mb, int l, int M, int* slice_rows) {
  const int K = mb.kpad[l], N = mb.npad[l], nb = (N % 128 == 0 && K % 128 == 0) ? 128 : 64;
  return dw_slices(c.force_slices, c.num_cus, M, (N / nb) * (K / nb), slice_rows);
}

// Lays a network's buffers out from byte offset `off` of the arena at `base` (nullptr: sizes only).  4 KiB granules, the
// alignment of an allocation of its own: with 256-byte granules the launch-bound [36, 224, 224, 224, 6] network took 21.09 ms
// of device time per epoch (batch 2048, 95 000 rows) against 20.70 with these and 20.72 with one hipMalloc per buffer.
inline size_t layout_member(const TrainCommon& c, Member& mb, char* base, size_t off) {
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += (bytes + 4095) & ~(size_t)4095; return p; };
  const int L = c.L;
  const size_t Mmax = (size_t)max_rows(c, c.cap_batch);   // the unstructured forms stack one pass: half the workspaces; a tangent handle three blocks
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
  mb.mem.partial = (double*)take((size_t)c.cap_batch / 64 * 8 * (c.tan ? 2 : 1));   // a tangent handle: the tangent partials behind the primal ones
  mb.mem.loss = (double*)take(24);                          // L, and under the tangent loss mse and tan_mse
  return off;
}

// Host Keras-order weights -> the padded device images (both layouts) of layer l.
inline int upload_layer(const TrainCommon& c, Member& mb, int l, const double* W, const double* b) {
  const int kp = mb.kpad[l], np_ = mb.npad[l], di = mb.dims[l], dn = mb.dims[l + 1];
  std::vector<float> wt((size_t)np_ * kp, 0.f), wk((size_t)kp * np_, 0.f), bb(np_, 0.f);
  for (int i = 0; i < di; ++i)
    for (int o = 0; o < dn; ++o) {
      const float w = (float)W[(size_t)i * dn + o];
      wt[(size_t)o * kp + i] = w; wk[(size_t)i * np_ + o] = w;
    }
  if (has_bias(c.form, c.L, l)) for (int o = 0; o < dn; ++o) bb[o] = (float)b[o];
  HIPCHK(hipMemcpy(mb.lay[l].Wt, wt.data(), wt.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(mb.lay[l].Wk, wk.data(), wk.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(mb.lay[l].b, bb.data(), bb.size() * 4, hipMemcpyHostToDevice));
  return NNMPC_OK;
}
// Every layer, then the snapshot: it starts as the initial weights.
inline int upload_member(const TrainCommon& c, Member& mb, const double* const* W, const double* const* b) {
  for (int l = 0; l < c.L; ++l)
    if (int rc = upload_layer(c, mb, l, W[l], b[l])) return rc;
  HIPCHK(hipMemcpy(mb.snap, mb.param, mb.param_floats * 4, hipMemcpyDeviceToDevice));
  return NNMPC_OK;
}
inline int set_weights(const char* who, const TrainCommon& c, Member& mb, const double* const* W, const double* const* b) {
  for (int l = 0; l < c.L; ++l)
    if (!W[l] || (has_bias(c.form, c.L, l) && !b[l])) { set_error("%s: missing weights or bias of layer %d", who, l); return NNMPC_EINVAL; }
  HIPCHK(hipSetDevice(c.device));
  HIPCHK(stream_sync(c.stream));
  for (int l = 0; l < c.L; ++l)
    if (int rc = upload_layer(c, mb, l, W[l], b[l])) return rc;
  return NNMPC_OK;
}

// The reverse, for the weights (grads == nullptr) or a summed gradient (per layer gW [N][K] then gb [N], back to back): the
// padded [out][in] image and the vector of every layer -> the host's Keras-order W[l], b[l].  A null host pointer is
// skipped; the head has a bias in the unstructured forms only.  The caller has waited for the stream.
inline int read_back(const TrainCommon& c, const Member& mb, const float* grads, double* const* W, double* const* b) {
  std::vector<float> tmp;
  for (int l = 0; l < c.L; ++l) {
    const int kp = mb.kpad[l], np_ = mb.npad[l], di = mb.dims[l], dn = mb.dims[l + 1];
    const size_t plane = (size_t)np_ * kp;
    const float* dW = grads ? grads : mb.lay[l].Wt;
    const float* db = grads ? grads + plane : mb.lay[l].b;
    if (grads) grads += plane + np_;
    if (W && W[l]) {
      tmp.resize(plane);
      HIPCHK(hipMemcpy(tmp.data(), dW, plane * 4, hipMemcpyDeviceToHost));
      for (int i = 0; i < di; ++i)
        for (int o = 0; o < dn; ++o) W[l][(size_t)i * dn + o] = (double)tmp[(size_t)o * kp + i];
    }
    if (b && has_bias(c.form, c.L, l) && b[l]) {
      tmp.resize(np_);
      HIPCHK(hipMemcpy(tmp.data(), db, (size_t)np_ * 4, hipMemcpyDeviceToHost));
      for (int o = 0; o < dn; ++o) b[l][o] = (double)tmp[o];
    }
  }
  return NNMPC_OK;
}
inline int get_weights(const TrainCommon& c, const Member& mb, double* const* W, double* const* b) {
  HIPCHK(hipSetDevice(c.device));
  HIPCHK(stream_sync(c.stream));
  return read_back(c, mb, nullptr, W, b);
}

// Folds the largest |padding entry| of a network's weights, biases and moments into *mx (a NaN counts, and stays).
inline int padding_scan(const TrainCommon& c, const Member& mb, double* mx) {
  std::vector<float> tmp;
  auto fold = [&](float v) { const double a = fabs((double)v); if (*mx == *mx && !(a <= *mx)) *mx = a; };
  for (int l = 0; l < c.L; ++l) {
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
      for (int o = (has_bias(c.form, c.L, l) ? dn : 0); o < np_; ++o) fold(tmp[o]);   // a bias-free head: the whole image
    }
  }
  return NNMPC_OK;
}

// One device-side copy: a network's weights of every layer lie back to back, the snapshot in the same layout.
inline int copy_params(const TrainCommon& c, Member& mb, bool to_snapshot) {
  HIPCHK(hipMemcpyAsync(to_snapshot ? mb.snap : mb.param, to_snapshot ? mb.param : mb.snap, mb.param_floats * 4,
                        hipMemcpyDeviceToDevice, c.stream));
  return NNMPC_OK;
}

// ---- dataset, uploads, events ----

__global__ void train_cvt_k(float* __restrict__ d, const double* __restrict__ s, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n; i += (size_t)gridDim.x * blockDim.x) d[i] = (float)s[i];
}

// One f32 column of cnt entries from f64 on the host or (ptr_kind NNMPC_DEVICE) already in HBM; the caller waits for the stream.
inline int upload_column(TrainCommon& c, float** d, const double* s, size_t cnt, int32_t ptr_kind, std::vector<float>& tmp) {
  if (int rc = c.res.alloc(d, cnt)) return rc;
  if (ptr_kind == NNMPC_HOST) {
    tmp.resize(cnt);
    for (size_t i = 0; i < cnt; ++i) tmp[i] = (float)s[i];
    HIPCHK(hipMemcpy(*d, tmp.data(), cnt * 4, hipMemcpyHostToDevice));
  } else {
    hipLaunchKernelGGL(train_cvt_k, dim3(1024), dim3(256), 0, c.stream, *d, s, cnt);
  }
  return NNMPC_OK;
}
inline void drop_tangents(TrainCommon& c) {
  for (float** p : {&c.tdx, &c.tdup, &c.tdxs, &c.tdus, &c.tt}) { c.res.give_back(*p); *p = nullptr; }
}

// The f32 dataset from f64 columns on the host or (ptr_kind NNMPC_DEVICE) already in HBM.  Tangents of the earlier dataset go with it.
inline int set_data(const char* who, TrainCommon& c, int32_t n, const double* x, const double* uprev, const double* xs,
                    const double* us, const double* u, int32_t ptr_kind) {
  if (n < 1 || !x || !xs || !us || !u) { set_error("%s: bad arguments", who); return NNMPC_EINVAL; }
  if (c.with_uprev && !uprev) { set_error("%s: uprev is an input of the network, none given", who); return NNMPC_EINVAL; }
  HIPCHK(hipSetDevice(c.device));
  HIPCHK(stream_sync(c.stream));
  for (float** p : {&c.dx, &c.dup, &c.dxs, &c.dus, &c.du}) { c.res.give_back(*p); *p = nullptr; }
  drop_tangents(c);
  c.n = 0;
  struct { float** d; const double* s; int w; } col[5] = {{&c.dx, x, c.nx}, {&c.dup, c.with_uprev ? uprev : nullptr, c.nu},
                                                          {&c.dxs, xs, c.nx}, {&c.dus, us, c.nu}, {&c.du, u, c.nu}};
  std::vector<float> tmp;
  for (auto& k : col) {
    if (!k.s) continue;
    if (int rc = upload_column(c, k.d, k.s, (size_t)n * k.w, ptr_kind, tmp)) return rc;
  }
  HIPCHK(stream_sync(c.stream));
  HIPCHK(hipGetLastError());
  c.n = n;
  return NNMPC_OK;
}

// The dataset's tangent directions and targets (a tangent handle only): `dirs` per row of the dataset set_data gave, every
// column [n][dirs][width]; dxs / dus on a whole-input handle and only there.
inline int set_tangents(const char* who, TrainCommon& c, int32_t n, int32_t dirs, const double* dx, const double* duprev,
                        const double* dxs, const double* dus, const double* t, int32_t ptr_kind) {
  if (!c.tan) { set_error("%s: a plain handle has no tangent loss (nnmpc_train_create_tan builds the handle that has)", who); return NNMPC_EINVAL; }
  if (dirs != c.tan_dirs) { set_error("%s: %d directions per row, the handle was built for %d", who, dirs, c.tan_dirs); return NNMPC_EINVAL; }
  if (int rc = check_data(c, who)) return rc;
  if (!dx || !t) { set_error("%s: bad arguments", who); return NNMPC_EINVAL; }
  if (n != c.n) { set_error("%s: tangents of %d rows for a dataset of %d", who, n, c.n); return NNMPC_EINVAL; }
  if (c.with_uprev && !duprev) { set_error("%s: uprev is an input of the network, no duprev given", who); return NNMPC_EINVAL; }
  if (c.tan_whole && (!dxs || !dus)) { set_error("%s: a whole-input handle takes dxs and dus", who); return NNMPC_EINVAL; }
  if (!c.tan_whole && (dxs || dus)) { set_error("%s: dxs / dus given, the handle's directions are [dx, (duprev)] only (whole_input = 1 at create builds the handle that takes them)", who); return NNMPC_EINVAL; }
  HIPCHK(hipSetDevice(c.device));
  HIPCHK(stream_sync(c.stream));
  drop_tangents(c);
  struct { float** d; const double* s; int w; } col[5] = {{&c.tdx, dx, c.nx}, {&c.tdup, c.with_uprev ? duprev : nullptr, c.nu},
                                                          {&c.tdxs, dxs, c.nx}, {&c.tdus, dus, c.nu}, {&c.tt, t, c.nu}};
  std::vector<float> tmp;
  for (auto& k : col) {
    if (!k.s) continue;
    if (int rc = upload_column(c, k.d, k.s, (size_t)n * dirs * k.w, ptr_kind, tmp)) { drop_tangents(c); return rc; }
  }
  HIPCHK(stream_sync(c.stream));
  HIPCHK(hipGetLastError());
  return NNMPC_OK;
}
// grad, step, epoch and eval of a handle whose loss has the tangent term need the tangents (before any launch).
inline int check_tangents(const TrainCommon& c, const char* who) {
  if (tan_active(c) && !c.tt) { set_error("%s: the tangent weight is %g and the dataset has no tangents (set_tangents comes after set_data, which drops them)", who, c.tan_w); return NNMPC_EINVAL; }
  return NNMPC_OK;
}

// A call's step table (tb bytes; a single handle has none) and, behind it, its row lists go to c.dcall in ONE copy out of a
// pinned image, so `rows` may be reused as soon as the call returns and the upload is a true asynchronous copy.  Two images
// are used in turn; before one is overwritten the host waits for the upload that last read it (two calls back), never for
// the kernels of the previous call.
inline int staged_upload(TrainCommon& c, const void* tab, size_t tb, const int32_t* rows, size_t nrows) {
  const size_t bytes = tb + nrows * 4;
  if (bytes > c.res.slots[0].cap) HIPCHK(stream_sync(c.stream));   // the slot is about to grow: nothing may still read the old buffer
  if (int rc = c.res.slot(0, &c.dcall, bytes)) return rc;
  const int k = c.stage_turn;
  c.stage_turn ^= 1;
  if (!c.stage_done[k]) { if (int rc = c.res.event(&c.stage_done[k], hipEventDisableTiming)) return rc; }
  else HIPCHK(hipEventSynchronize(c.stage_done[k]));
  char* img = nullptr;
  if (int rc = c.res.pinned_slot(k, &img, bytes)) return rc;
  if (tb) memcpy(img, tab, tb);
  if (nrows) memcpy(img + tb, rows, nrows * 4);
  HIPCHK(hipMemcpyAsync(c.dcall, img, bytes, hipMemcpyHostToDevice, c.stream));
  HIPCHK(hipEventRecord(c.stage_done[k], c.stream));
  return NNMPC_OK;
}

// n doubles from the device, after everything enqueued so far.
inline int read_doubles(const TrainCommon& c, const double* src, double* out, size_t n) {
  HIPCHK(hipMemcpyAsync(out, src, n * 8, hipMemcpyDeviceToHost, c.stream));
  HIPCHK(stream_sync(c.stream));
  HIPCHK(hipGetLastError());
  return NNMPC_OK;
}

struct EvSet { hipEvent_t f0, f1, b0, b1; };                // around the forward GEMMs; around the backward up to, not including, Adam
inline int ev_set(TrainCommon& c, size_t i, EvSet* e) {
  if (int rc = c.res.pool_event(4 * i + 3, &e->b1)) return rc;
  const hipEvent_t* ev = c.res.pool.data() + 4 * i;
  *e = EvSet{ev[0], ev[1], ev[2], ev[3]};
  return NNMPC_OK;
}
// hipEvent ms of the last call: the spans of its c.nsets event sets, and e0 .. e1.
inline int last_ms(TrainCommon& c, double* gemm_ms, double* total_ms) {
  HIPCHK(hipSetDevice(c.device));
  HIPCHK(stream_sync(c.stream));
  double g = 0.0;
  float ms = 0.f;
  const std::vector<hipEvent_t>& ev = c.res.pool;
  for (size_t i = 0; i < c.nsets && 4 * i + 3 < ev.size(); ++i) {
    if (hipEventElapsedTime(&ms, ev[4 * i], ev[4 * i + 1]) == hipSuccess) g += ms;
    if (hipEventElapsedTime(&ms, ev[4 * i + 2], ev[4 * i + 3]) == hipSuccess) g += ms;
  }
  ms = 0.f;
  if (c.nsets) hipEventElapsedTime(&ms, c.e0, c.e1);
  if (gemm_ms) *gemm_ms = g;
  if (total_ms) *total_ms = ms;
  return NNMPC_OK;
}

}  // namespace
}  // namespace nnmpc
