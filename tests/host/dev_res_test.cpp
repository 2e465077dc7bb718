// DevRes and Staging (csrc/dev_res.h) against a fake HIP runtime: one scripted life of an owner, and one host-pointer call
// of three segments through the staging helper, each run clean and then once for every k with the k-th fake call failing.  Links nothing from ROCm: the HIP entry points the header calls are defined here over
// malloc, with a set of live objects per kind.  Built and run by tests/test_cpu_dev_res.py:
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I<rocm>/include -I<csrc> -I<include> dev_res_test.cpp
#include "dev_res.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <set>
#include <string>

using namespace nnmpc;

// ---- the fake runtime ----
namespace {
std::set<void*> g_dev, g_host, g_events, g_streams;         // live objects per kind
int g_calls = 0, g_fail_at = 0;                             // calls that can fail so far; the one that does (0: none)
const char* g_failed = nullptr;                             // the call that did
int g_bad_frees = 0, g_mallocs = 0, g_syncs = 0, g_copies = 0;
size_t g_last_bytes = 0;
unsigned g_last_flags = 0;
char g_err[512];

bool fails(const char* what) {
  if (++g_calls != g_fail_at) return false;
  g_failed = what;
  return true;
}
hipError_t make(std::set<void*>& live, void** out, size_t bytes) {
  *out = malloc(bytes ? bytes : 1);
  memset(*out, 0xAB, bytes);                                // not zero: the owner's memset has to do that
  live.insert(*out);
  return hipSuccess;
}
hipError_t drop(std::set<void*>& live, void* p) {
  if (!live.erase(p)) { ++g_bad_frees; return hipErrorInvalidValue; }   // freed twice, or never made
  free(p);
  return hipSuccess;
}
}  // namespace

char* nnmpc::error_buffer() { return g_err; }

extern "C" {
hipError_t hipMalloc(void** p, size_t n) {
  if (fails("hipMalloc")) return hipErrorOutOfMemory;
  ++g_mallocs; g_last_bytes = n;
  return make(g_dev, p, n);
}
hipError_t hipFree(void* p) { return drop(g_dev, p); }
hipError_t hipMemset(void* p, int v, size_t n) {
  if (fails("hipMemset")) return hipErrorInvalidValue;
  memset(p, v, n);
  return hipSuccess;
}
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) {
  if (fails("hipMemcpy")) return hipErrorInvalidValue;
  memcpy(d, s, n);
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) {
  if (fails("hipMemcpyAsync")) return hipErrorInvalidValue;
  ++g_copies;
  memcpy(d, s, n);
  return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t n, unsigned int flags) {
  if (fails("hipHostMalloc")) return hipErrorOutOfMemory;
  g_last_bytes = n; g_last_flags = flags;
  return make(g_host, p, n);
}
hipError_t hipHostFree(void* p) { return drop(g_host, p); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
  if (fails("hipEventCreateWithFlags")) return hipErrorOutOfMemory;
  g_last_flags = flags;
  return make(g_events, (void**)e, 1);
}
hipError_t hipEventCreate(hipEvent_t* e) { return hipEventCreateWithFlags(e, 0); }
hipError_t hipEventDestroy(hipEvent_t e) { return drop(g_events, e); }
hipError_t hipStreamCreate(hipStream_t* s) {
  if (fails("hipStreamCreate")) return hipErrorOutOfMemory;
  return make(g_streams, (void**)s, 1);
}
hipError_t hipStreamDestroy(hipStream_t s) { return drop(g_streams, s); }
hipError_t hipStreamQuery(hipStream_t) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { ++g_syncs; return hipSuccess; }
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "fake failure"; }
}

// ---- the script ----
namespace {
int g_checks = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { fprintf(stderr, "dev_res_test: line %d (fail_at %d, failed %s): %s\n", __LINE__, g_fail_at, g_failed ? g_failed : "-", #c); exit(1); } } while (0)

// After a step of the script that returned rc: true if it went through.  If the fake failure fell into it, the code is the
// documented one (an allocation: NNMPC_ENOMEM; anything else: NNMPC_EHIP) and there is an error text.
bool went_through(int rc, const char* failed_before) {
  if (g_failed == failed_before) { CHECK(rc == NNMPC_OK); return true; }
  const bool alloc = !strcmp(g_failed, "hipMalloc") || !strcmp(g_failed, "hipHostMalloc");
  CHECK(rc == (alloc ? NNMPC_ENOMEM : NNMPC_EHIP));
  CHECK(g_err[0] != 0);
  return false;
}
#define STEP(call) (g_err[0] = 0, before = g_failed, went_through((call), before))

size_t live() { return g_dev.size() + g_host.size() + g_events.size() + g_streams.size(); }

// One life of an owner with the fail_at-th fake call failing (0: none).  Returns the number of fake calls that can fail.
int life(int fail_at) {
  g_calls = 0; g_fail_at = fail_at; g_failed = nullptr; g_bad_frees = 0; g_syncs = 0;
  const char* before = nullptr;
  {
    DevRes r(2, 1);
    r.device = 3;
    double* const sentinel = (double*)0x10;

    // allocations: zeroed, max(count, 1) elements, the output untouched on failure
    double* a = sentinel;
    if (STEP(r.alloc(&a, 10))) {
      CHECK(g_dev.count(a) && g_last_bytes == 80);
      for (int i = 0; i < 10; ++i) CHECK(a[i] == 0.0);
    } else CHECK(a == sentinel && g_dev.empty());
    int* z = (int*)sentinel;
    if (STEP(r.alloc(&z, 0))) CHECK(g_dev.count(z) && g_last_bytes == sizeof(int) && *z == 0);
    else CHECK(z == (int*)sentinel);

    // upload
    const float src[5] = {1.f, 2.f, 3.f, 4.f, 5.f};
    float* u = (float*)sentinel;
    const size_t dev_before = g_dev.size();
    if (STEP(r.upload(&u, src, 5))) CHECK(g_dev.count(u) && !memcmp(u, src, sizeof src));
    else { CHECK(u == (float*)sentinel && g_dev.size() == dev_before); u = nullptr; }   // the half-made buffer went back at once

    // a slot grows, holds, is not shrunk, grows again: one rule, the old buffer freed first
    char *s0 = nullptr, *s1 = nullptr;
    if (STEP(r.slot(0, &s0, 1000))) {
      CHECK(r.slots[0].cap == 1000 + 250 + 256 && g_last_bytes == r.slots[0].cap && s0 == r.slots[0].p);
      const int m = g_mallocs;
      CHECK(r.slot(0, &s1, 1000) == NNMPC_OK && s1 == s0 && g_mallocs == m);            // the same size again: no hipMalloc
      CHECK(r.slot(0, &s1, 10) == NNMPC_OK && s1 == s0 && g_mallocs == m && r.slots[0].cap == 1506);
      CHECK(r.slot(0, &s1, 1506) == NNMPC_OK && s1 == s0 && g_mallocs == m);            // up to the capacity
    } else CHECK(!r.slots[0].p && r.slots[0].cap == 0 && !s0);
    const size_t dev_mid = g_dev.size();
    if (STEP(r.slot(0, &s1, 5000))) CHECK(r.slots[0].cap == 5000 + 1250 + 256 && g_dev.size() == (s0 ? dev_mid : dev_mid + 1));   // (the new buffer may lie where the old one did)
    else CHECK(!r.slots[0].p && r.slots[0].cap == 0 && !g_dev.count(s0));                // freed before the new one was asked for
    if (STEP(r.slot(1, &s1, 0))) CHECK(!s1 && !r.slots[1].p);                            // nothing asked for, nothing made
    g_err[0] = 0;
    CHECK(r.slot(2, &s1, 8) == NNMPC_EINVAL && g_err[0]);                                // the handle fixed two slots

    // pinned: a slot (the same rule) and an allocation, default flags
    char* p0 = nullptr;
    if (STEP(r.pinned_slot(0, &p0, 100))) CHECK(g_host.count(p0) && r.pinned_slots[0].cap == 100 + 25 + 256 && g_last_flags == hipHostMallocDefault);
    else CHECK(!p0 && g_host.empty());
    int* pa = (int*)sentinel;
    if (STEP(r.pinned_alloc(&pa, 4))) CHECK(g_host.count(pa) && g_last_bytes == 16);
    else CHECK(pa == (int*)sentinel);

    // streams and events
    hipStream_t st[2] = {nullptr, nullptr};
    for (hipStream_t& s : st)
      if (STEP(r.stream(&s))) CHECK(g_streams.count(s)); else CHECK(!s);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (STEP(r.event(&e0))) CHECK(g_events.count(e0) && g_last_flags == hipEventDefault); else CHECK(!e0);
    if (STEP(r.event(&e1, hipEventDisableTiming))) CHECK(g_events.count(e1) && g_last_flags == hipEventDisableTiming); else CHECK(!e1);

    // the pool: event 0, then event 9; it stops at the first failure and holds created events only
    hipEvent_t pe = nullptr;
    if (STEP(r.pool_event(0, &pe))) CHECK(r.pool.size() == 1 && pe == r.pool[0]); else CHECK(r.pool.empty() && !pe);
    const size_t had = r.pool.size();
    pe = nullptr;
    if (STEP(r.pool_event(9, &pe))) CHECK(r.pool.size() == 10 && pe == r.pool[9]); else CHECK(r.pool.size() >= had && r.pool.size() < 10 && !pe);
    for (hipEvent_t e : r.pool) CHECK(e && g_events.count(e));
    if (r.pool.size() == 10) { const int c = g_calls; CHECK(r.pool_event(4, &pe) == NNMPC_OK && pe == r.pool[4] && g_calls == c); }

    // give one buffer back; a pointer the owner does not hold is an error return
    if (u) { CHECK(r.give_back(u) == NNMPC_OK && !g_dev.count(u)); }
    int local = 0;
    g_err[0] = 0;
    CHECK(r.give_back(&local) == NNMPC_EINVAL && g_err[0] && g_bad_frees == 0);
    if (u) CHECK(r.give_back(u) == NNMPC_EINVAL);                                          // given back already
    CHECK(r.give_back(nullptr) == NNMPC_OK);

    // release, twice, then the destructor
    const bool held = live() != 0;
    r.release();
    CHECK(live() == 0 && g_bad_frees == 0 && g_syncs == (held ? 1 : 0));
    r.release();
    CHECK(g_bad_frees == 0 && g_syncs == (held ? 1 : 0));
  }
  CHECK(live() == 0 && g_bad_frees == 0);
  if (fail_at) CHECK(g_failed != nullptr);                  // the switch did fire
  return g_calls;
}

// One host-pointer call through Staging with the fail_at-th fake call failing (0: none): B = 5 rows in segments of 2, 2 and 1.
// x (3 doubles a row) is an input in a slot, w (1 double a row) an input in a buffer the handle owns, y (2 ints a row) an
// output, k (1 int a row) an output the "kernel" needs though the caller passes none, and one input and one output are null.
// Returns the number of fake calls that can fail.
int staged_call(int fail_at) {
  g_calls = 0; g_fail_at = fail_at; g_failed = nullptr; g_bad_frees = 0;
  const char* before = nullptr;
  enum { S_X = 0, S_Y, S_K, S_NULL_IN, S_NULL_OUT, S_COUNT };
  const int B = 5, G = 2;
  double x[B * 3], w[B];
  int y[(B + 1) * 2];
  for (int i = 0; i < B * 3; ++i) x[i] = 10.0 * (i / 3) + i % 3;
  for (int i = 0; i < B; ++i) w[i] = 100.0 * i;
  for (int& v : y) v = -7;
  {
    DevRes r(S_COUNT);
    double* fixed = nullptr;
    bool ok = STEP(r.alloc(&fixed, G));
    Staging st{r, nullptr, true};
    int done = 0;                                           // rows delivered
    for (int b0 = 0; b0 < B && ok; b0 += G) {
      const int nb = std::min(G, B - b0);
      const double *xd = nullptr, *wd = nullptr, *none_in = (const double*)0x10;
      int *yd = nullptr, *kd = nullptr, *none_out = (int*)0x10;
      const int mallocs = g_mallocs;
      ok = STEP(st.in(&xd, x, b0, nb, 3, S_X)) && STEP(st.in(&wd, w, b0, nb, 1, S_NULL_IN, fixed)) &&
           STEP(st.in(&none_in, (const double*)nullptr, b0, nb, 3, S_NULL_IN)) && STEP(st.out(&yd, y, b0, nb, 2, S_Y)) &&
           STEP(st.out(&kd, (int*)nullptr, b0, nb, 1, S_K, true)) && STEP(st.out(&none_out, (int*)nullptr, b0, nb, 2, S_NULL_OUT));
      if (!ok) break;
      CHECK(xd == r.slots[S_X].p && wd == fixed && yd == r.slots[S_Y].p && kd == r.slots[S_K].p && kd);
      CHECK(!none_in && !none_out && !r.slots[S_NULL_IN].p && !r.slots[S_NULL_OUT].p);   // null optionals: no pointer, no slot
      if (b0) CHECK(g_mallocs == mallocs);                  // the first segment is the largest: no slot grows after it
      CHECK(!memcmp(xd, x + b0 * 3, nb * 3 * sizeof(double)) && !memcmp(wd, w + b0, nb * sizeof(double)));   // inputs are in already
      CHECK(st.npending == 1);                              // y alone goes back
      for (int i = 0; i < nb; ++i) {                        // the "kernel"
        kd[i] = (int)wd[i] + 1;
        for (int j = 0; j < 2; ++j) yd[i * 2 + j] = (int)xd[i * 3 + j] + kd[i];
      }
      CHECK(y[b0 * 2] == -7);                               // nothing before copy_out
      const int copies = g_copies;
      ok = STEP(st.copy_out());
      if (ok) { CHECK(g_copies == copies + 1 && st.npending == 0); done = b0 + nb; }
    }
    if (ok) CHECK(done == B);
    for (int i = 0; i < done; ++i)
      for (int j = 0; j < 2; ++j) CHECK(y[i * 2 + j] == 10 * i + j + 100 * i + 1);
    for (int i = done * 2; i < (B + 1) * 2; ++i) CHECK(y[i] == -7);   // rows not delivered, and the row past B, untouched

    // device pointers: offsets of the caller's own, no slot, no copy; a kept output the caller did not pass still gets its slot
    if (ok) {
      DevRes r2(S_COUNT);
      Staging dv{r2, nullptr, false};
      const int copies = g_copies, calls = g_calls;
      const double *xd = nullptr, *none_in = (const double*)0x10;
      int *yd = nullptr, *none_out = (int*)0x10, *kd = nullptr;
      CHECK(dv.in(&xd, x, 2, 2, 3, S_X) == NNMPC_OK && xd == x + 6);
      CHECK(dv.in(&xd, x, 2, 2, 3, S_X, fixed) == NNMPC_OK && xd == x + 6);
      CHECK(dv.in(&none_in, (const double*)nullptr, 2, 2, 3, S_NULL_IN) == NNMPC_OK && !none_in);
      CHECK(dv.out(&yd, y, 4, 1, 2, S_Y) == NNMPC_OK && yd == y + 8);
      CHECK(dv.out(&yd, y, 4, 1, 2, S_Y, true) == NNMPC_OK && yd == y + 8);
      CHECK(dv.out(&none_out, (int*)nullptr, 4, 1, 2, S_NULL_OUT) == NNMPC_OK && !none_out);
      CHECK(dv.copy_out() == NNMPC_OK && g_copies == copies && g_calls == calls && dv.npending == 0);
      for (const DevRes::Slot& s : r2.slots) CHECK(!s.p);
      if (STEP(dv.out(&kd, (int*)nullptr, 4, 1, 1, S_K, true))) CHECK(kd && kd == r2.slots[S_K].p);
      else CHECK(!kd && !r2.slots[S_K].p);
      CHECK(dv.copy_out() == NNMPC_OK && g_copies == copies);
    }
  }
  CHECK(live() == 0 && g_bad_frees == 0);                   // the owner released everything, whichever step failed
  if (fail_at) CHECK(g_failed != nullptr);
  return g_calls;
}

// More outputs than a call can hold pending is an error return, not a write past the array.
void staging_bounds() {
  g_fail_at = 0;
  DevRes r(1);
  Staging st{r, nullptr, true};
  int y[4] = {0, 0, 0, 0}, *d = nullptr;
  const int cap = (int)(sizeof st.pending / sizeof st.pending[0]);
  for (int i = 0; i < cap; ++i) CHECK(st.out(&d, y, 0, 1, 4, 0) == NNMPC_OK);
  g_err[0] = 0;
  CHECK(st.out(&d, y, 0, 1, 4, 0) == NNMPC_EINVAL && g_err[0] && st.npending == cap);
}

// An owner that is only destroyed releases too.
void destructor_releases() {
  g_fail_at = 0;
  {
    DevRes r(1);
    int* a = nullptr; char* s = nullptr; hipStream_t st; hipEvent_t e;
    CHECK(r.alloc(&a, 3) == NNMPC_OK && r.slot(0, &s, 64) == NNMPC_OK && r.stream(&st) == NNMPC_OK && r.pool_event(1, &e) == NNMPC_OK);
    CHECK(live() == 5);
  }
  CHECK(live() == 0 && g_bad_frees == 0);
}
}  // namespace

int main() {
  const int n = life(0);
  CHECK(n >= 25);                                           // every step of the script reached the fake runtime
  for (int k = 1; k <= n; ++k) life(k);
  destructor_releases();
  const int m = staged_call(0);
  CHECK(m >= 1 + 3 + 3 * 2 + 3);                            // the buffer, three slots, two copies in a segment, three out
  for (int k = 1; k <= m; ++k) staged_call(k);
  staging_bounds();
  printf("dev_res_test: ok (%d + %d fake calls failed in turn, %d checks)\n", n, m, g_checks);
  return 0;
}
