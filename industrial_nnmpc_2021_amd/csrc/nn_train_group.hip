// A sweep of networks of one form trained in lock step for gfx950: the step of nn_train.hip with the member network as a
// grid coordinate, so a layer of G networks is one launch (one per tile class present) instead of G.  This file holds the
// grouped kernels, their enqueue order, the per-call step table and the nnmpc_train_group_* entry points; a member's
// layout, padding, uploads, read-backs, the dataset, events and argument checks are nn_train_host.h's, shared with the
// single-network handle.
//
// Members share nx, nu, with_uprev, the depth, the form, max_batch, the Adam hyper-parameters and ONE f32 dataset; they differ in
// widths, weights, rows, Adam step count and snapshot.  In lock-step step k member g works on its batch k (B rows; B = 0:
// the member has run out of rows, or sits this call out, and every workgroup of its grid plane returns at once).
//
// A member's bytes do not depend on the rest of the group and equal what an nnmpc_train handle gives: every kernel here is
// the workgroup function of nn_train_dev.h that the single-network kernel runs, at the member's own block coordinates and
// with the member's own shapes (padding, tile class, dW slices from its own M and tile count); the scalars of a step (Adam
// bias corrections from the member's own t, loss scales) are computed on the host in double as nn_train.hip computes them
// and travel in a table uploaded once per call with the row lists.  No atomics, no hand-off between workgroups.
//
// The form (NNMPC_NN_*) is one per group and travels by value in GShape, so it is uniform per launch: the unstructured forms
// gather one row per sample (train_gather_rows1), stack M = train_rows(form, Bp) = Bp rows wherever the structured form stacks
// 2 Bp, run the head with its bias (and ReLU) in the GEMM epilogue, take pred from the head as it is (train_output1_block) and
// add the head's bias column sums and bias Adam: 6 L + 2 launches per lock-step step against 6 L.
//
// The tangent loss (nnmpc_train_create_group_tan, structured form): every member carries its OWN weight w[g] >= 0 of the
// tangent term; the tangents are shared as the data is.  A member with w[g] > 0 stacks 3 Bp rows in its steps (GStep.tan)
// and runs what a tangent handle of nn_train.hip runs -- both gathers, the pair tile on the hidden layers, the head over
// 3 Bp rows, the tangent output block and loss finish, dW over 3 Bp rows, the bias column sums over 2 Bp, dA with the mask
// wrapped to the pass-1 rows -- each inside the launch the plain members share, so a step keeps its 6 L launches whatever
// the mix of weights.  A member with w[g] == 0 runs the plain step over 2 Bp rows: the bytes of a member of a plain group.
//
// Device tables:  GLayer [G][L] and GMember [G], written at create (pointers, padded K and N);  GStep [steps][G], per call.
#include "nn_train_host.h"

using namespace nnmpc;

namespace {

struct GStep {                                              // member g in lock-step step k
  AdamCoef k;                                               // from the member's own step count
  double loss_scale, acc_w;
  double w;                                                 // the member's tangent weight (the loss finish: L = mse + w tan_mse)
  float gscale, gw;                                         // gw = (float)(gscale in double * w), as nn_train.hip rounds it
  int B, at;                                                // rows of the batch (0: inactive); position in the row lists, or first dataset row
  int tan, pad_;                                            // 1: the member stacks the tangent rows in this step (w > 0 in a tangent group)
};
struct GShape { int nx, nu, with_uprev, L, force_slices, num_cus, form, cap; };   // cap: cap_batch (the tangent partials lie cap / 64 behind the primal ones)
struct GData { const float *x, *uprev, *xs, *us, *u, *tdx, *tdup, *tt; };

__device__ __forceinline__ int pad128(int B) { return ((B + 127) / 128) * 128; }
// Stacked rows of member g's batch in this step: 3 Bp with the tangent rows, else train_rows.
__device__ __forceinline__ int member_rows(const GShape& sh, const GStep& s) { return train_rows_tan(sh.form, pad128(s.B), s.tan); }
// Block (bx, by) of a member's own ntn x ntm extent -> its tile, as gemm_nt_f32_k remaps it (row panels of 8 back to back: a
// bijection of the extent; which workgroup computes a tile changes no sum).
__device__ __forceinline__ void remap_tile(int ntn, int ntm, int bx, int by, int* tm, int* tn) {
  const int bid = bx + ntn * by, full = (ntm >> 3) * 8 * ntn;
  if (bid < full) { const int sq = bid >> 3; *tm = (sq / ntn) * 8 + (bid & 7); *tn = sq % ntn; }
  else { const int rem = bid - full; *tm = (ntm >> 3) * 8 + rem / ntn; *tn = rem % ntn; }
}

// Grid (row blocks, G).
__global__ __launch_bounds__(128) void grp_gather_k(const GLayer* __restrict__ lay, const GStep* __restrict__ st, GShape sh,
                                                    GData d, const int* __restrict__ rows) {
  const int g = blockIdx.y, B = st[g].B;
  if (B == 0) return;
  const GLayer& ld = lay[(size_t)g * sh.L];
  if (sh.form == NNMPC_NN_STRUCTURED) {
    train_gather_rows(ld.ain, ld.K, pad128(B), B, sh.nx, sh.nu, sh.with_uprev, d.x, d.uprev, d.xs, d.us,
                      rows ? rows + st[g].at : nullptr, st[g].at, blockIdx.x, gridDim.x);
    if (st[g].tan)                                          // train_gather_tan_k: the third block behind the two (one direction, partial input)
      train_gather_tan_rows(ld.ain, ld.K, pad128(B), B, sh.nx, sh.nu, sh.with_uprev, 1, 0, d.tdx, d.tdup, nullptr, nullptr,
                            rows ? rows + st[g].at : nullptr, st[g].at, blockIdx.x, gridDim.x);
  } else
    train_gather_rows1(ld.ain, ld.K, pad128(B), B, sh.nx, sh.nu, sh.with_uprev, d.x, d.uprev, d.xs, d.us,
                       rows ? rows + st[g].at : nullptr, st[g].at, blockIdx.x, gridDim.x);
}

// Layer l forward for the members whose N is in tile class NB.  Grid (max N / NB, max M / NB, G); inside a member's own
// ntn x ntm extent the workgroup id is remapped (remap_tile).  The head of a tangent member runs here over its 3 Bp rows.
template <int NB, bool RELU, bool BIAS>
__global__ __launch_bounds__(256) void grp_fwd_k(const GLayer* __restrict__ lay, const GStep* __restrict__ st, GShape sh, int l) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int g = blockIdx.z, B = st[g].B;
  if (B == 0) return;
  const GLayer& ld = lay[(size_t)g * sh.L + l];
  if ((ld.N % 128 == 0) != (NB == 128)) return;
  const int ntn = ld.N / NB, ntm = member_rows(sh, st[g]) / NB;
  if ((int)blockIdx.x >= ntn || (int)blockIdx.y >= ntm) return;
  int tm, tn;
  remap_tile(ntn, ntm, blockIdx.x, blockIdx.y, &tm, &tn);
  train_fwd_tile<NB, RELU, BIAS>(ld.aout, ld.N, ld.ain, ld.K, ld.Wt, ld.K, ld.K, ld.b, tm, tn, lds);
}

// A hidden layer's forward when a tangent member is active in tile class NB: launched INSTEAD of grp_fwd_k<NB, true, true>,
// so a layer stays one launch per tile class whatever the mix of weights.  A tangent member does what gemm_nt_f32_pair_k
// does: row tiles below Bp / NB are a pass-1 tile with its tangent tile (train_fwd_pair_tile), those in [Bp / NB, 2 Bp / NB)
// the plain tile of pass 2, and it has none beyond.  A plain member (w == 0) never enters the pair tile: it runs
// grp_fwd_k's own lines over its 2 Bp rows.  Grid (max N / NB, max 2 Bp / NB, G); structured form only.
template <int NB>
__global__ __launch_bounds__(256) void grp_fwd_pair_k(const GLayer* __restrict__ lay, const GStep* __restrict__ st, GShape sh, int l) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int g = blockIdx.z, B = st[g].B;
  if (B == 0) return;
  const GLayer& ld = lay[(size_t)g * sh.L + l];
  if ((ld.N % 128 == 0) != (NB == 128)) return;
  const int Bp = pad128(B), ntn = ld.N / NB, ntm = 2 * Bp / NB;
  if ((int)blockIdx.x >= ntn || (int)blockIdx.y >= ntm) return;
  int tm = blockIdx.y, tn = blockIdx.x;
  if (st[g].tan) {
    if (tm < Bp / NB) {
      train_fwd_pair_tile<NB>(ld.aout, ld.N, ld.ain, ld.K, ld.Wt, ld.K, ld.K, ld.b, Bp, tm, tn, lds);
      return;
    }
  } else {
    remap_tile(ntn, ntm, blockIdx.x, blockIdx.y, &tm, &tn);
  }
  train_fwd_tile<NB, true, true>(ld.aout, ld.N, ld.ain, ld.K, ld.Wt, ld.K, ld.K, ld.b, tm, tn, lds);
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
  if (st[g].tan)                                            // train_output_tan_k; the tangent partials behind the primal ones
    train_output_tan_block(backward ? mem[g].dz[0] : nullptr, ld.aout, ld.N, Bp, B, sh.nu, 1, 0, d.us, d.u, d.tt, nullptr,
                           rows ? rows + st[g].at : nullptr, st[g].at, st[g].gscale, st[g].gw, mem[g].partial,
                           mem[g].partial + sh.cap / 64, blockIdx.x);
  else if (sh.form == NNMPC_NN_STRUCTURED)
    train_output_block(backward ? mem[g].dz[0] : nullptr, ld.aout, ld.N, Bp, B, sh.nu, d.us, d.u,
                       rows ? rows + st[g].at : nullptr, st[g].at, st[g].gscale, mem[g].partial, blockIdx.x);
  else
    train_output1_block(backward ? mem[g].dz[0] : nullptr, ld.aout, ld.N, B, sh.nu, sh.form == NNMPC_NN_UNSTD_RELU, d.u,
                        rows ? rows + st[g].at : nullptr, st[g].at, st[g].gscale, mem[g].partial, blockIdx.x);
}

// Grid (G): one thread per member.  A member owns three acc words (L, mse, tan_mse); a plain member uses the first.
__global__ void grp_loss_finish_k(const GMember* __restrict__ mem, const GStep* __restrict__ st, int cap) {
  const int g = blockIdx.x, B = st[g].B;
  if (threadIdx.x != 0 || B == 0) return;
  if (st[g].tan)
    train_loss_finish_tan(mem[g].partial, mem[g].partial + cap / 64, pad128(B) / 64, st[g].loss_scale, st[g].loss_scale, st[g].acc_w, st[g].w,
                          mem[g].loss, mem[g].acc);
  else
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
  const int M = member_rows(sh, st[g]);
  int slice_rows = 0;
  if (s >= layer_slices(ld, sh, M, &slice_rows)) return;
  train_tn_tile<NB>(ld.planes, (size_t)ld.N * ld.K, (size_t)ld.K, mem[g].dz[cur], (size_t)ld.N, ld.ain, (size_t)ld.K, M,
                    slice_rows, blockIdx.x, blockIdx.y, s, lds);
}

// Grid (max N / 64, max train_rows / 128, G): never the tangent rows, which carry no bias gradient.
__global__ __launch_bounds__(256) void grp_colsum_k(const GLayer* __restrict__ lay, const GMember* __restrict__ mem,
                                                    const GStep* __restrict__ st, GShape sh, int l, int cur) {
  const int g = blockIdx.z, B = st[g].B;
  if (B == 0) return;
  const GLayer& ld = lay[(size_t)g * sh.L + l];
  if ((int)blockIdx.x >= ld.N / 64 || (int)blockIdx.y >= train_rows(sh.form, pad128(B)) / 128) return;
  train_colsum_block(ld.bplanes, mem[g].dz[cur], ld.N, blockIdx.x, blockIdx.y);
}

// dZ_{l-1} of layer l for the members whose K is in tile class NB.  Grid (max K / NB, max M / NB, G).  A tangent member's
// row tiles at or above 2 Bp take their mask 2 Bp rows up, from the pass-1 rows (gemm_nt_mask_wrap_k).
template <int NB>
__global__ __launch_bounds__(256) void grp_da_k(const GLayer* __restrict__ lay, const GMember* __restrict__ mem,
                                                const GStep* __restrict__ st, GShape sh, int l, int cur) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int g = blockIdx.z, B = st[g].B;
  if (B == 0) return;
  const GLayer& ld = lay[(size_t)g * sh.L + l];
  if ((ld.K % 128 == 0) != (NB == 128)) return;
  if ((int)blockIdx.x >= ld.K / NB || (int)blockIdx.y >= member_rows(sh, st[g]) / NB) return;
  const int wrap = 2 * pad128(B);
  const float* mask = (st[g].tan && (int)blockIdx.y * NB >= wrap) ? ld.ain - (size_t)wrap * ld.K : ld.ain;
  train_nt_mask_tile<NB>(mem[g].dz[cur ^ 1], (size_t)ld.K, mem[g].dz[cur], (size_t)ld.N, ld.Wk, (size_t)ld.N, ld.N, mask,
                         blockIdx.x, blockIdx.y, lds);
}

// Grid (max K / 64, max N / 64, G).
__global__ __launch_bounds__(256) void grp_adam_w_k(const GLayer* __restrict__ lay, const GStep* __restrict__ st, GShape sh, int l) {
  const int g = blockIdx.z, B = st[g].B;
  if (B == 0) return;
  const GLayer& ld = lay[(size_t)g * sh.L + l];
  if ((int)blockIdx.x >= ld.K / 64 || (int)blockIdx.y >= ld.N / 64) return;
  int slice_rows = 0;
  const int S = layer_slices(ld, sh, member_rows(sh, st[g]), &slice_rows);
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
  if (i < ld.N) ld.b[i] = adam_entry(plane_sum(ld.bplanes, (size_t)ld.N, train_rows(sh.form, pad128(B)) / 128, (size_t)i), ld.mb + i, ld.vb + i, ld.b[i], k);
}

}  // namespace

struct nnmpc_train_group {
  TrainCommon c;
  int G = 0;
  std::vector<Member> m;
  char* arena = nullptr;                                    // every per-member buffer
  GLayer* dlay = nullptr; GMember* dmem = nullptr;          // the device tables
  double* dacc = nullptr;                                   // acc of every member (L, mse, tan_mse: 3 words each), contiguous: one read per call
  int64_t launches = 0;                                     // kernels enqueued by the last epoch / eval
  std::vector<double> w;                                    // a tangent group (c.tan): the members' own weights of the tangent term
  // What nnmpc_train_last_group_losses returns: the sums of the last epoch / eval, the member's denominator (0: it had no
  // rows) and whether it stacked the tangent rows (its words are L, mse, tan_mse; otherwise L alone, which is the mse).
  bool has_last = false;
  std::vector<double> last_sum, last_den;
  std::vector<char> last_tan;
};

namespace {

// Every kernel of a call goes through here: the count is what nnmpc_train_group_last_launches reports.
template <class... P, class... A>
void launch(nnmpc_train_group* h, void (*k)(P...), dim3 grid, dim3 block, size_t lds, A... args) {
  ++h->launches;
  hipLaunchKernelGGL(k, grid, block, lds, h->c.stream, args...);
}

// The forward instance of a layer, as nn_train.hip picks it: relu and bias on the hidden layers; on the head neither
// (structured), the bias (NNMPC_NN_UNSTD) or both (NNMPC_NN_UNSTD_RELU: the hidden layers' instance).
// pair: a tangent member is active in this class on a hidden layer, so the launch is grp_fwd_pair_k (in its place, not beside it).
template <int NB>
void launch_fwd(nnmpc_train_group* h, dim3 grid, bool relu, bool bias, bool pair, const GStep* st, const GShape& sh, int l) {
  const size_t lds = TileCfg<NB>::LDS_FLOATS * 4;
  if (pair) launch(h, grp_fwd_pair_k<NB>, grid, dim3(256), lds, h->dlay, st, sh, l);
  else if (relu) launch(h, grp_fwd_k<NB, true, true>, grid, dim3(256), lds, h->dlay, st, sh, l);
  else if (bias) launch(h, grp_fwd_k<NB, false, true>, grid, dim3(256), lds, h->dlay, st, sh, l);
  else launch(h, grp_fwd_k<NB, false, false>, grid, dim3(256), lds, h->dlay, st, sh, l);
}

// One lock-step step on the handle's stream: gather, forward, output, and (backward) the gradient planes and Adam, for
// the members with host[g].B > 0.  st: this step's row of the device table; rows: the device row lists, or nullptr (eval).
int enqueue_step(nnmpc_train_group* h, const GStep* host, const GStep* st, const int* rows, bool backward, size_t set) {
  TrainCommon& c = h->c;
  const int G = h->G, L = c.L;
  const GShape sh{c.nx, c.nu, c.with_uprev, L, c.force_slices, c.num_cus, c.form, c.cap_batch};
  const GData d{c.dx, c.dup, c.dxs, c.dus, c.du, c.tdx, c.tdup, c.tt};
  int Bpmax = 0, Mmax = 0;                                  // Mmax: over the members' own stacked rows (3 Bp for those with the tangent rows)
  for (int g = 0; g < G; ++g) {
    Bpmax = std::max(Bpmax, pad128_host(host[g].B));
    Mmax = std::max(Mmax, train_rows_tan(c.form, pad128_host(host[g].B), host[g].tan));
  }
  if (Bpmax == 0) return NNMPC_OK;
  const int M2max = train_rows(c.form, Bpmax);              // without the tangent rows: the hidden layers' forward and the bias column sums
  EvSet e;
  if (int rc = ev_set(c, set, &e)) return rc;
  struct Ext { int n = 0, k = 0, s = 0; };                  // largest extents of a tile class (0: 64, 1: 128) among the active members; 0: class absent
  launch(h, grp_gather_k, dim3(std::min(Bpmax, 2048), G), dim3(128), 0, h->dlay, st, sh, d, rows);
  hipEventRecord(e.f0, c.stream);
  for (int l = 0; l < L; ++l) {
    const bool last = l == L - 1, relu = !last || c.form == NNMPC_NN_UNSTD_RELU;
    int nmax[2] = {0, 0};
    bool pair[2] = {false, false};                          // a hidden layer with a tangent member active in the class
    for (int g = 0; g < G; ++g)
      if (host[g].B) {
        const int N = h->m[g].npad[l], big = N % 128 == 0;
        nmax[big] = std::max(nmax[big], N);
        if (host[g].tan && !last) pair[big] = true;
      }
    const int rows_l = last ? Mmax : M2max;                 // the head runs over a tangent member's 3 Bp rows, a hidden layer over 2 Bp
    if (nmax[1]) launch_fwd<128>(h, dim3(nmax[1] / 128, rows_l / 128, G), relu, has_bias(c.form, L, l), pair[1], st, sh, l);
    if (nmax[0]) launch_fwd<64>(h, dim3(nmax[0] / 64, rows_l / 64, G), relu, has_bias(c.form, L, l), pair[0], st, sh, l);
  }
  hipEventRecord(e.f1, c.stream);
  launch(h, grp_output_k, dim3(Bpmax / 64, G), dim3(256), 0, h->dlay, h->dmem, st, sh, d, rows, backward ? 1 : 0);
  launch(h, grp_loss_finish_k, dim3(G), dim3(64), 0, h->dmem, st, c.cap_batch);
  hipEventRecord(e.b0, c.stream);
  if (backward) {
    int cur = 0;
    for (int l = L - 1; l >= 0; --l) {
      Ext dw[2], da[2];
      int nall = 0;
      for (int g = 0; g < G; ++g) {
        if (!host[g].B) continue;
        const Member& mb = h->m[g];
        const int K = mb.kpad[l], N = mb.npad[l];
        const int big = N % 128 == 0 && K % 128 == 0;
        int slice_rows = 0;
        const int S = member_slices(c, mb, l, train_rows_tan(c.form, pad128_host(host[g].B), host[g].tan), &slice_rows);
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
      if (has_bias(c.form, L, l)) launch(h, grp_colsum_k, dim3(nall / 64, M2max / 128, G), dim3(256), 0, h->dlay, h->dmem, st, sh, l, cur);
      if (l > 0) {
        if (da[1].k) launch(h, grp_da_k<128>, dim3(da[1].k / 128, Mmax / 128, G), dim3(256), TileCfg<128>::LDS_FLOATS * 4,
                            h->dlay, h->dmem, st, sh, l, cur);
        if (da[0].k) launch(h, grp_da_k<64>, dim3(da[0].k / 64, Mmax / 64, G), dim3(256), TileCfg<64>::LDS_FLOATS * 4,
                            h->dlay, h->dmem, st, sh, l, cur);
        cur ^= 1;
      }
    }
  }
  hipEventRecord(e.b1, c.stream);
  if (backward)
    for (int l = 0; l < L; ++l) {
      int nall = 0, kall = 0;
      for (int g = 0; g < G; ++g)
        if (host[g].B) { nall = std::max(nall, h->m[g].npad[l]); kall = std::max(kall, h->m[g].kpad[l]); }
      launch(h, grp_adam_w_k, dim3(kall / 64, nall / 64, G), dim3(256), 0, h->dlay, st, sh, l);
      if (has_bias(c.form, L, l)) launch(h, grp_adam_b_k, dim3((nall + 255) / 256, G), dim3(256), 0, h->dlay, st, sh, l);
    }
  return NNMPC_OK;
}

// The call's steps on the stream between e0 and e1, then the members' acc words in one read.  tab: the GStep table
// (steps x G), already on the device at c.dcall with the row lists behind it (with_rows) or without any (eval).
int run_call(nnmpc_train_group* h, const std::vector<GStep>& tab, int steps, bool with_rows, bool backward, std::vector<double>& sum) {
  TrainCommon& c = h->c;
  const int G = h->G;
  const GStep* dtab = (const GStep*)c.dcall;
  const int* drows = with_rows ? (const int*)(c.dcall + tab.size() * sizeof(GStep)) : nullptr;
  HIPCHK(hipMemsetAsync(h->dacc, 0, (size_t)G * 24, c.stream));
  hipEventRecord(c.e0, c.stream);
  for (int k = 0; k < steps; ++k)
    if (int rc = enqueue_step(h, &tab[(size_t)k * G], dtab + (size_t)k * G, drows, backward, k)) return rc;
  c.nsets = steps;
  hipEventRecord(c.e1, c.stream);
  sum.assign((size_t)3 * G, 0.0);                           // member g: sum[3 g] = L, and with the tangent rows mse and tan_mse behind it
  return read_doubles(c, h->dacc, sum.data(), (size_t)3 * G);
}

// The tangent scalars of member g's step of B rows, as enqueue_batch of nn_train.hip forms them: gs in double, gw = (float)(gs w).
void step_tan(const nnmpc_train_group* h, GStep& s, int g, int B) {
  const double w = h->c.tan ? h->w[g] : 0.0, gs = 2.0 / ((double)B * h->c.nu);
  s.gscale = (float)gs;
  s.tan = w > 0.0 ? 1 : 0;
  s.w = w;
  s.gw = (float)(gs * w);
}

// A member whose loss has the tangent term needs the tangents (before any launch), as check_tangents for a single handle.
int check_group_tangents(const nnmpc_train_group* h, const char* who) {
  if (!h->c.tan || h->c.tt) return NNMPC_OK;
  for (int g = 0; g < h->G; ++g)
    if (h->w[g] > 0.0) { set_error("%s: member %d: the tangent weight is %g and the dataset has no tangents (nnmpc_train_set_group_tangents comes after nnmpc_train_group_set_data, which drops them)", who, g, h->w[g]); return NNMPC_EINVAL; }
  return NNMPC_OK;
}

// What nnmpc_train_last_group_losses reads: the call's sums, per member its denominator (0: no rows) and whether its words are three.
void keep_last(nnmpc_train_group* h, const std::vector<double>& sum, const std::vector<double>& den) {
  h->has_last = true;
  h->last_sum = sum; h->last_den = den;
  h->last_tan.assign(h->G, 0);
  for (int g = 0; g < h->G; ++g) h->last_tan[g] = h->c.tan && h->w[g] > 0.0;
}

int check_member(const nnmpc_train_group* h, const char* who, int g) {
  if (g < 0 || g >= h->G) { set_error("%s: member %d of a group of %d", who, g, h->G); return NNMPC_EINVAL; }
  return NNMPC_OK;
}
}  // namespace

extern "C" {

int nnmpc_train_group_destroy(nnmpc_train_group* h) {
  if (!h) return NNMPC_OK;
  h->c.res.release();
  delete h;
  return NNMPC_OK;
}

// The create entry points; `who` is the one that was called.  tan: a tangent group (nnmpc_train_create_group_tan).
static int group_create(const char* who, nnmpc_train_group** out, int32_t G, int32_t nlayers, const int32_t* dims,
                        const double* const* W, const double* const* b, int32_t nx, int32_t nu, int32_t with_uprev,
                        int32_t max_batch, double lr, double beta1, double beta2, double eps, int32_t form, bool tan = false) {
  GUARD_BEGIN
  if (!out || nlayers < 1 || !dims || !W || !b || nx <= 0 || nu <= 0 || max_batch < 1) { set_error("%s: bad arguments", who); return NNMPC_EINVAL; }
  if (G < 1) { set_error("%s: a group of %d networks", who, G); return NNMPC_EINVAL; }
  if (int rc = check_form(who, form)) return rc;
  if (tan && form != NNMPC_NN_STRUCTURED) { set_error("%s: form %d: the tangent loss is built for the structured form only (NNMPC_NN_STRUCTURED)", who, form); return NNMPC_EINVAL; }
  const int L = nlayers;
  for (int g = 0; g < G; ++g) {
    char mem[32];
    snprintf(mem, sizeof mem, "member %d: ", g);
    if (int rc = check_network(who, mem, L, dims + (size_t)g * (L + 1), W + (size_t)g * L, b + (size_t)g * L, nx, nu, with_uprev, form)) return rc;
  }
  if (int rc = check_adam(who, lr, beta1, beta2, eps)) return rc;
  if (int rc = check_device(who)) return rc;
  Building<nnmpc_train_group, nnmpc_train_group_destroy> guard(new nnmpc_train_group());
  nnmpc_train_group* h = guard.get();
  TrainCommon& c = h->c;
  if (int rc = common_init(who, c, L, nx, nu, with_uprev, max_batch, lr, beta1, beta2, eps, form)) return rc;
  h->G = G;
  c.tan = tan ? 1 : 0;                                      // before the shapes: workspaces, planes and slices for 3 cap_batch rows
  h->w.assign(G, 0.0);
  if (tan) { HIPCHK(hipFuncSetAttribute((const void*)grp_fwd_pair_k<128>, hipFuncAttributeMaxDynamicSharedMemorySize, TileCfg<128>::LDS_FLOATS * 4)); }
  HIPCHK(hipFuncSetAttribute((const void*)grp_fwd_k<128, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, TileCfg<128>::LDS_FLOATS * 4));
  HIPCHK(hipFuncSetAttribute((const void*)grp_fwd_k<128, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, TileCfg<128>::LDS_FLOATS * 4));
  HIPCHK(hipFuncSetAttribute((const void*)grp_fwd_k<128, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, TileCfg<128>::LDS_FLOATS * 4));   // the unstructured linear head
  HIPCHK(hipFuncSetAttribute((const void*)grp_da_k<128>, hipFuncAttributeMaxDynamicSharedMemorySize, TileCfg<128>::LDS_FLOATS * 4));
  HIPCHK(hipFuncSetAttribute((const void*)grp_dw_k<128>, hipFuncAttributeMaxDynamicSharedMemorySize, TileCfgTN<128>::LDS_FLOATS * 4));
  h->m.resize(G);
  size_t bytes = 0;
  for (int g = 0; g < G; ++g) {
    Member& mb = h->m[g];
    member_shapes(c, mb, dims + (size_t)g * (L + 1));
    bytes = layout_member(c, mb, nullptr, bytes);
    for (int S : mb.max_slices)                             // the dW grid carries member x slice in z
      if ((int64_t)G * S > 65535) { set_error("%s: %d members x %d dW slices exceed a grid's z extent", who, G, S); return NNMPC_EINVAL; }
  }
  if (int rc = c.res.alloc(&h->arena, bytes)) return rc;
  if (int rc = c.res.alloc(&h->dacc, (size_t)3 * G)) return rc;
  std::vector<GLayer> lay;
  std::vector<GMember> mem;
  size_t off = 0;
  for (int g = 0; g < G; ++g) {
    Member& mb = h->m[g];
    off = layout_member(c, mb, h->arena, off);
    mb.mem.acc = h->dacc + 3 * g;
    if (int rc = upload_member(c, mb, W + (size_t)g * L, b + (size_t)g * L)) return rc;
    lay.insert(lay.end(), mb.lay.begin(), mb.lay.end());
    mem.push_back(mb.mem);
  }
  if (int rc = c.res.upload(&h->dlay, lay.data(), lay.size())) return rc;
  if (int rc = c.res.upload(&h->dmem, mem.data(), mem.size())) return rc;
  *out = guard.release();
  return NNMPC_OK;
  GUARD_END
}

int nnmpc_train_group_create(nnmpc_train_group** out, int32_t G, int32_t nlayers, const int32_t* dims, const double* const* W,
                             const double* const* b, int32_t nx, int32_t nu, int32_t with_uprev, int32_t max_batch,
                             double lr, double beta1, double beta2, double eps) {
  return group_create(__func__, out, G, nlayers, dims, W, b, nx, nu, with_uprev, max_batch, lr, beta1, beta2, eps, NNMPC_NN_STRUCTURED);
}

int nnmpc_train_create_group_ex(nnmpc_train_group** out, int32_t G, int32_t nlayers, const int32_t* dims, const double* const* W,
                                const double* const* b, int32_t nx, int32_t nu, int32_t with_uprev, int32_t max_batch,
                                double lr, double beta1, double beta2, double eps, int32_t form) {
  return group_create(__func__, out, G, nlayers, dims, W, b, nx, nu, with_uprev, max_batch, lr, beta1, beta2, eps, form);
}

int nnmpc_train_create_group_tan(nnmpc_train_group** out, int32_t G, int32_t nlayers, const int32_t* dims, const double* const* W,
                                 const double* const* b, int32_t nx, int32_t nu, int32_t with_uprev, int32_t max_batch,
                                 double lr, double beta1, double beta2, double eps, int32_t form) {
  return group_create(__func__, out, G, nlayers, dims, W, b, nx, nu, with_uprev, max_batch, lr, beta1, beta2, eps, form, true);
}

int nnmpc_train_set_group_tangents(nnmpc_train_group* h, int32_t n, const double* dx, const double* duprev, const double* t, int32_t ptr_kind) {
  GUARD_BEGIN
  if (!h) { set_error("nnmpc_train_set_group_tangents: bad arguments"); return NNMPC_EINVAL; }
  return set_tangents(__func__, h->c, n, 1, dx, duprev, nullptr, nullptr, t, ptr_kind);
  GUARD_END
}

int nnmpc_train_set_group_tan_weights(nnmpc_train_group* h, const double* w) {
  if (!h || !w) { set_error("nnmpc_train_set_group_tan_weights: bad arguments"); return NNMPC_EINVAL; }
  if (!h->c.tan) { set_error("nnmpc_train_set_group_tan_weights: a plain group has no tangent loss (nnmpc_train_create_group_tan builds the group that has)"); return NNMPC_EINVAL; }
  for (int g = 0; g < h->G; ++g)
    if (!(w[g] >= 0.0) || !isfinite(w[g])) { set_error("nnmpc_train_set_group_tan_weights: member %d: weight %g (finite and >= 0)", g, w[g]); return NNMPC_EINVAL; }
  h->w.assign(w, w + h->G);
  return NNMPC_OK;
}

int nnmpc_train_last_group_losses(nnmpc_train_group* h, double* mse, double* tan_mse) {
  if (!h) { set_error("nnmpc_train_last_group_losses: bad arguments"); return NNMPC_EINVAL; }
  if (!h->has_last) { set_error("nnmpc_train_last_group_losses: no epoch or eval yet"); return NNMPC_EINVAL; }
  for (int g = 0; g < h->G; ++g) {
    const double den = h->last_den[g], *v = &h->last_sum[(size_t)3 * g];
    if (mse) mse[g] = den > 0.0 ? (h->last_tan[g] ? v[1] : v[0]) / den : NAN;   // without the tangent term the loss is the mse
    if (tan_mse) tan_mse[g] = den > 0.0 ? (h->last_tan[g] ? v[2] / den : 0.0) : NAN;
  }
  return NNMPC_OK;
}

int nnmpc_train_group_set_data(nnmpc_train_group* h, int32_t n, const double* x, const double* uprev, const double* xs,
                               const double* us, const double* u, int32_t ptr_kind) {
  GUARD_BEGIN
  if (!h) { set_error("nnmpc_train_group_set_data: bad arguments"); return NNMPC_EINVAL; }
  return set_data(__func__, h->c, n, x, uprev, xs, us, u, ptr_kind);
  GUARD_END
}

int nnmpc_train_group_epoch(nnmpc_train_group* h, const int32_t* nrows, const int32_t* perm, int32_t batch, double* loss) {
  GUARD_BEGIN
  if (!h || !nrows || !perm) { set_error("nnmpc_train_group_epoch: bad arguments"); return NNMPC_EINVAL; }
  TrainCommon& c = h->c;
  if (int rc = check_batch(c, __func__, batch)) return rc;
  const int G = h->G;
  size_t total = 0;
  int steps = 0;
  for (int g = 0; g < G; ++g) {
    if (nrows[g] < 0) { set_error("nnmpc_train_group_epoch: member %d: %d rows", g, nrows[g]); return NNMPC_EINVAL; }
    total += (size_t)nrows[g];
    steps = std::max(steps, (nrows[g] + batch - 1) / batch);
  }
  if (total > (size_t)INT32_MAX) { set_error("nnmpc_train_group_epoch: %zu rows in all, at most 2^31 - 1", total); return NNMPC_EINVAL; }
  if (int rc = check_rows(c, __func__, total, perm)) return rc;
  if (int rc = check_group_tangents(h, __func__)) return rc;
  if (loss) for (int g = 0; g < G; ++g) loss[g] = NAN;      // a member without rows has no loss
  h->launches = 0; c.nsets = 0;
  std::vector<double> den(G);
  for (int g = 0; g < G; ++g) den[g] = (double)nrows[g];
  if (steps == 0) { keep_last(h, std::vector<double>((size_t)3 * G, 0.0), den); return NNMPC_OK; }
  HIPCHK(hipSetDevice(c.device));
  // the table: per member the batches of nnmpc_train_epoch (the last one is the short one), each with the scalars of its own Adam step
  std::vector<GStep> tab((size_t)steps * G, GStep{});
  size_t at = 0;
  for (int g = 0; g < G; ++g) {
    for (int i = 0, k = 0; i < nrows[g]; i += batch, ++k) {
      GStep& s = tab[(size_t)k * G + g];
      const int B = std::min(batch, nrows[g] - i);
      s.k = adam_coef(c.lr, c.beta1, c.beta2, c.eps, h->m[g].t + k + 1);
      s.loss_scale = 1.0 / ((double)B * c.nu); s.acc_w = (double)B;
      step_tan(h, s, g, B);
      s.B = B; s.at = (int)(at + i);
    }
    at += nrows[g];
  }
  if (int rc = staged_upload(c, tab.data(), tab.size() * sizeof(GStep), perm, total)) return rc;
  for (int g = 0; g < G; ++g) h->m[g].t += (nrows[g] + batch - 1) / batch;
  std::vector<double> sum;
  if (int rc = run_call(h, tab, steps, true, true, sum)) return rc;
  keep_last(h, sum, den);
  if (loss) for (int g = 0; g < G; ++g) if (nrows[g]) loss[g] = sum[(size_t)3 * g] / (double)nrows[g];
  return NNMPC_OK;
  GUARD_END
}

int nnmpc_train_group_eval(nnmpc_train_group* h, const int32_t* first, const int32_t* count, double* mse) {
  GUARD_BEGIN
  if (!h || !first || !count || !mse) { set_error("nnmpc_train_group_eval: bad arguments"); return NNMPC_EINVAL; }
  TrainCommon& c = h->c;
  if (int rc = check_data(c, __func__)) return rc;
  const int G = h->G;
  int steps = 0;
  for (int g = 0; g < G; ++g) {
    if (count[g] < 0 || (count[g] > 0 && (first[g] < 0 || (int64_t)first[g] + count[g] > c.n))) {
      set_error("nnmpc_train_group_eval: member %d: rows [%d, %d + %d) outside [0, %d)", g, first[g], first[g], count[g], c.n); return NNMPC_EINVAL;
    }
    steps = std::max(steps, (count[g] + c.max_batch - 1) / c.max_batch);
  }
  if (int rc = check_group_tangents(h, __func__)) return rc;
  for (int g = 0; g < G; ++g) mse[g] = NAN;                 // a member without rows has no loss
  h->launches = 0; c.nsets = 0;
  std::vector<double> den(G);
  for (int g = 0; g < G; ++g) den[g] = (double)count[g] * c.nu;
  if (steps == 0) { keep_last(h, std::vector<double>((size_t)3 * G, 0.0), den); return NNMPC_OK; }
  HIPCHK(hipSetDevice(c.device));
  std::vector<GStep> tab((size_t)steps * G, GStep{});
  for (int g = 0; g < G; ++g)
    for (int i = 0, k = 0; i < count[g]; i += c.max_batch, ++k) {
      GStep& s = tab[(size_t)k * G + g];
      const int B = std::min(c.max_batch, count[g] - i);
      s.loss_scale = 1.0; s.acc_w = 1.0;
      step_tan(h, s, g, B);
      s.B = B; s.at = first[g] + i;
    }
  if (int rc = staged_upload(c, tab.data(), tab.size() * sizeof(GStep), nullptr, 0)) return rc;
  std::vector<double> sum;
  if (int rc = run_call(h, tab, steps, false, false, sum)) return rc;
  keep_last(h, sum, den);
  for (int g = 0; g < G; ++g) if (count[g]) mse[g] = sum[(size_t)3 * g] / ((double)count[g] * c.nu);
  return NNMPC_OK;
  GUARD_END
}

int nnmpc_train_group_get_weights(nnmpc_train_group* h, int32_t g, double* const* W, double* const* b) {
  GUARD_BEGIN
  if (!h || !W || !b) { set_error("nnmpc_train_group_get_weights: bad arguments"); return NNMPC_EINVAL; }
  if (int rc = check_member(h, __func__, g)) return rc;
  return get_weights(h->c, h->m[g], W, b);
  GUARD_END
}

int nnmpc_train_group_set_weights(nnmpc_train_group* h, int32_t g, const double* const* W, const double* const* b) {
  GUARD_BEGIN
  if (!h || !W || !b) { set_error("nnmpc_train_group_set_weights: bad arguments"); return NNMPC_EINVAL; }
  if (int rc = check_member(h, __func__, g)) return rc;
  return set_weights(__func__, h->c, h->m[g], W, b);
  GUARD_END
}

static int copy_masked(nnmpc_train_group* h, const char* who, const int32_t* mask, bool to_snapshot) {
  if (!h || !mask) { set_error("%s: bad arguments", who); return NNMPC_EINVAL; }
  HIPCHK(hipSetDevice(h->c.device));
  for (int g = 0; g < h->G; ++g)
    if (mask[g])
      if (int rc = copy_params(h->c, h->m[g], to_snapshot)) return rc;
  return NNMPC_OK;
}

int nnmpc_train_group_snapshot(nnmpc_train_group* h, const int32_t* mask) { return copy_masked(h, __func__, mask, true); }

int nnmpc_train_group_restore(nnmpc_train_group* h, const int32_t* mask) { return copy_masked(h, __func__, mask, false); }

int nnmpc_train_group_last_ms(nnmpc_train_group* h, double* gemm_ms, double* total_ms) {
  if (!h) { set_error("nnmpc_train_group_last_ms: bad arguments"); return NNMPC_EINVAL; }
  return last_ms(h->c, gemm_ms, total_ms);
}

int nnmpc_train_group_last_launches(nnmpc_train_group* h, int64_t* n) {
  if (!h || !n) { set_error("nnmpc_train_group_last_launches: bad arguments"); return NNMPC_EINVAL; }
  *n = h->launches;
  return NNMPC_OK;
}

int nnmpc_train_group_padding_max(nnmpc_train_group* h, double* maxabs) {
  GUARD_BEGIN
  if (!h || !maxabs) { set_error("nnmpc_train_group_padding_max: bad arguments"); return NNMPC_EINVAL; }
  HIPCHK(hipSetDevice(h->c.device));
  HIPCHK(stream_sync(h->c.stream));
  *maxabs = 0.0;
  for (const Member& mb : h->m)
    if (int rc = padding_scan(h->c, mb, maxabs)) return rc;
  return NNMPC_OK;
  GUARD_END
}

}  // extern "C"
