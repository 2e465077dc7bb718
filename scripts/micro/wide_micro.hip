// Stand-alone timing and check of the far-field full-width GEMM with its epilogue: asm_wide_gemm_k<WIDE_FAR> (qp_wide.h).
//   wide_micro [rows] [column tiles] [nu] [window]      defaults: the headline's shape, 99200 31 32 512
// Synthetic T, U (staircase k averaging ~100 of 256), rowprob (a permutation of the problems, ~1 % of the rows -1), lb, ub.
// Prints ms per launch (hipEvents), checks u_out / st / wflag of a sample of rows against a host loop and prints a hash of
// the sampled outputs: two builds that agree bit for bit print the same hash.
// Build (from the repository root; binaries go to scripts/micro/run/):
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -mllvm -pragma-unroll-threshold=1000000 -I industrial_nnmpc_2021_amd/csrc \
//     scripts/micro/wide_micro.hip -o scripts/micro/run/wide_micro
//   -DWIDE_EPILOGUE_IMAGE=0   the epilogue without the LDS image of the bounds (one load round trip per row group): the A/B
//   -DASM_STAMPS [-DASM_STAMP_WG=<workgroup>]   s_memtime stamps of wave 0 of one workgroup: K loop, load phase, store phase
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include <cmath>
#include "qp_wide.h"
using namespace nnmpc;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static double urand() { return (rand() / (double)RAND_MAX) * 2 - 1; }

int main(int argc, char** argv) {
  const int rows = argc > 1 ? atoi(argv[1]) : 99200, ntn = argc > 2 ? atoi(argv[2]) : 31, nu = argc > 3 ? atoi(argv[3]) : 32;
  const int c0 = argc > 4 ? atoi(argv[4]) : 512, rp = 256;
  if (rows % 128 || c0 % 128 || nu < 1) { printf("rows and window: multiples of 128\n"); return 1; }
  const int ntm = rows / 128, n = c0 + 128 * ntn, nseg = rows;
  printf("rows %d (%d tiles)  columns %d beyond %d (%d tiles)  nu %d  image epilogue %d\n", rows, ntm, 128 * ntn, c0, ntn, nu, (int)WIDE_EPILOGUE_IMAGE);
  srand(7);
  std::vector<int> ffk(ntn), rowprob(rows);
  double kmean = 0;
  for (int t = 0; t < ntn; ++t) { ffk[t] = std::max(16, 16 * ((208 - 7 * t) / 16)); kmean += ffk[t]; }
  std::vector<double> hT((size_t)rows * rp), hU((size_t)128 * ntn * rp, 0.0), hlb((size_t)nseg * nu), hub((size_t)nseg * nu);
  for (auto& v : hT) v = 0.05 * urand();
  for (int c = 0; c < 128 * ntn; ++c)
    for (int k = 0; k < ffk[c / 128]; ++k) hU[(size_t)c * rp + k] = urand();
  for (size_t i = 0; i < hlb.size(); ++i) { hlb[i] = -(0.5 + 0.5 * fabs(urand())); hub[i] = 0.5 + 0.5 * fabs(urand()); }
  for (int r = 0; r < rows; ++r) rowprob[r] = r % 100 == 37 ? -1 : (int)(((long long)r * 7919) % nseg);   // (7919 is coprime to 99200)
  double flop = 0;
  for (int t = 0; t < ntn; ++t) flop += 2.0 * rows * 128 * ffk[t];
  printf("staircase k: mean %.1f of %d, %.3e flop, %.2f GB of u written\n", kmean / ntn, rp, flop, 8.0 * rows * 128 * ntn * 0.99 / 1e9);

  AsmDev d;
  memset(&d, 0, sizeof d);
  d.n = d.np = n; d.nu = nu; d.nseg = nseg; d.bound_tol = 1e-9;
  d.ffr = rp; d.ffW = c0; d.ldu = n; d.nout = n; d.wrows = rows;
  double *T, *U, *lb, *ub, *u; int *rpd, *kd, *wflag; unsigned char* st;
  CK(hipMalloc(&T, hT.size() * 8)); CK(hipMalloc(&U, hU.size() * 8)); CK(hipMalloc(&lb, hlb.size() * 8)); CK(hipMalloc(&ub, hub.size() * 8));
  CK(hipMalloc(&u, (size_t)nseg * n * 8)); CK(hipMalloc(&st, (size_t)nseg * n)); CK(hipMalloc(&wflag, (size_t)nseg * 4));
  CK(hipMalloc(&rpd, rows * 4)); CK(hipMalloc(&kd, ntn * 4));
  CK(hipMemcpy(T, hT.data(), hT.size() * 8, hipMemcpyHostToDevice)); CK(hipMemcpy(U, hU.data(), hU.size() * 8, hipMemcpyHostToDevice));
  CK(hipMemcpy(lb, hlb.data(), hlb.size() * 8, hipMemcpyHostToDevice)); CK(hipMemcpy(ub, hub.data(), hub.size() * 8, hipMemcpyHostToDevice));
  CK(hipMemcpy(rpd, rowprob.data(), rows * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(kd, ffk.data(), ntn * 4, hipMemcpyHostToDevice));
  CK(hipMemset(u, 0xff, (size_t)nseg * n * 8)); CK(hipMemset(st, 0, (size_t)nseg * n)); CK(hipMemset(wflag, 0, (size_t)nseg * 4));
  d.T = T; d.ffU = U; d.lb = lb; d.ub = ub; d.u_out = u; d.st = st; d.wflag = wflag; d.rowprob = rpd; d.ffk = kd;
  CK(hipFuncSetAttribute((const void*)asm_wide_gemm_k<WIDE_FAR>, hipFuncAttributeMaxDynamicSharedMemorySize, G64_LDS));
  auto run = [&] { hipLaunchKernelGGL(asm_wide_gemm_k<WIDE_FAR>, dim3(g64_grid(ntm, ntn)), dim3(256), G64_LDS, 0, d, c0, ntm, ntn); };
  run();
  CK(hipDeviceSynchronize());

  // ---- a sample of rows against the host: x = T U' in a plain loop (another summation order: 1e-12), the bound states and the flag
  // wherever x is not within 1e-12 of a threshold; rows without a problem leave no trace (the problems 37 * 7919 % nseg ... are theirs)
  {
    std::vector<double> ur(n); std::vector<unsigned char> sr(n);
    double md = 0; long bad = 0, viol = 0, ties = 0; uint64_t hash = 1469598103934665603ull;
    auto mix = [&](const void* p, size_t nb) { const unsigned char* c = (const unsigned char*)p; for (size_t i = 0; i < nb; ++i) { hash ^= c[i]; hash *= 1099511628211ull; } };
    for (int t = 0; t < 96; ++t) {
      const int row = t < 4 ? t * 42 + 1 : (int)(((long long)t * 1566083941ll) % rows);
      const int p = rowprob[row];
      if (p < 0) continue;
      int wf;
      CK(hipMemcpy(ur.data(), u + (size_t)p * n, n * 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(sr.data(), st + (size_t)p * n, n, hipMemcpyDeviceToHost));
      CK(hipMemcpy(&wf, wflag + p, 4, hipMemcpyDeviceToHost));
      mix(ur.data() + c0, (size_t)(n - c0) * 8); mix(sr.data(), n); mix(&wf, 4);
      int any = 0, tie = 0;
      for (int c = c0; c < n; ++c) {
        double s = 0;
        for (int k = 0; k < ffk[(c - c0) / 128]; ++k) s += hT[(size_t)row * rp + k] * hU[(size_t)(c - c0) * rp + k];
        md = fmax(md, fabs(s - ur[c]));
        const double hi = hub[(size_t)p * nu + c % nu] + d.bound_tol, lo = hlb[(size_t)p * nu + c % nu] - d.bound_tol;
        if (fabs(s - hi) < 1e-12 || fabs(s - lo) < 1e-12) { ++tie; continue; }
        const int ns = s > hi ? 1 : (s < lo ? 2 : 0);
        any |= ns; viol += ns != 0;
        if (sr[c] != ns) ++bad;
      }
      for (int c = 0; c < c0; ++c) if (sr[c] != 0) ++bad;                         // nothing inside the window is touched
      if (!tie && (wf != 0) != (any != 0)) ++bad;
      ties += tie;
    }
    // a problem no row points to: untouched
    {
      std::vector<char> used(nseg, 0);
      for (int r = 0; r < rows; ++r) if (rowprob[r] >= 0) used[rowprob[r]] = 1;
      int p = 0; while (p < nseg && used[p]) ++p;
      if (p < nseg) {
        CK(hipMemcpy(ur.data(), u + (size_t)p * n, n * 8, hipMemcpyDeviceToHost));
        for (int c = 0; c < n; ++c) { uint64_t w; memcpy(&w, &ur[c], 8); if (w != ~0ull) ++bad; }
      }
    }
    printf("check: max |host - u| %.3e  violations %ld  wrong st / wflag / untouched entries %ld  (near-ties skipped %ld)  hash %016llx  %s\n", md, viol, bad, ties,
           (unsigned long long)hash, md < 1e-12 && bad == 0 ? "OK" : "FAILED");
    if (!(md < 1e-12) || bad) return 2;
  }
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  for (int rep = 0; rep < 5; ++rep) {
    CK(hipEventRecord(e0));
    for (int i = 0; i < 5; ++i) run();
    CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1)); ms /= 5;
    printf("asm_wide_gemm_k<FAR>  %.3f ms  %.1f TFLOP/s  %.2f TB/s written\n", ms, flop / (ms * 1e-3) / 1e12, 8.0 * rows * 128 * ntn * 0.99 / (ms * 1e-3) / 1e12);
  }
#ifdef ASM_STAMPS
  {
    unsigned long long s_[64];
    CK(hipMemcpyFromSymbol(s_, HIP_SYMBOL(asm_stamp_buf), sizeof s_));
    printf("stamps of wave 0 of workgroup %d (s_memtime ticks): K loop %llu, load phase %llu, stores issued %llu, stores acknowledged %llu\n", (int)ASM_STAMP_WG,
           s_[1] - s_[0], s_[2] > s_[1] ? s_[2] - s_[1] : 0ull, s_[3] - (s_[2] > s_[1] ? s_[2] : s_[1]), s_[4] - s_[3]);
  }
#endif
  return 0;
}
