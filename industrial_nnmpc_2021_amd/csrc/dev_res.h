// What every handle of libnnmpc_hip.so owns on the device, in one place: the error macros, and DevRes -- the owner of a
// handle's device memory, pinned host memory, streams and events.  A handle holds one DevRes; its named pointers, streams
// and events are plain non-owning copies of what the owner made.  Staging forms the device pointers of a batched call's
// arguments on top of the owner's slots.  No kernels here: a host compiler builds this header.
#pragma once
#include <stddef.h>
#include <algorithm>
#include <memory>
#include <new>
#include <vector>
#include "../../include/nnmpc.h"
#include "common.h"

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { set_error("%s: %s", #x, hipGetErrorString(e_)); return NNMPC_EHIP; } } while (0)
// Around the body of an extern "C" entry point that can allocate host memory: no C++ exception crosses the C ABI.
#define GUARD_BEGIN try {
#define GUARD_END } catch (const std::bad_alloc&) { set_error("%s: out of host memory", __func__); return NNMPC_ENOMEM; } \
                    catch (...) { set_error("%s: unexpected exception", __func__); return NNMPC_EHIP; }

namespace nnmpc {

inline int check_device(const char* who) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { set_error("%s: no HIP device available (no CPU fallback)", who); return NNMPC_EHIP; }
  return NNMPC_OK;
}

struct DevRes {
  struct Slot { void* p = nullptr; size_t cap = 0; };
  int device = 0;                                           // the handle's create sets it; release() frees there
  std::vector<void*> mem, pinned;                           // alloc / upload; pinned_alloc
  std::vector<Slot> slots, pinned_slots;                    // grow-only, selected by index
  std::vector<hipEvent_t> events, pool;                     // event(); pool_event(i)
  std::vector<hipStream_t> streams;

  explicit DevRes(size_t nslots = 0, size_t npinned_slots = 0) : slots(nslots), pinned_slots(npinned_slots) {}
  DevRes(const DevRes&) = delete;
  DevRes& operator=(const DevRes&) = delete;
  ~DevRes() { release(); }

  // max(count, 1) zeroed elements of device memory; *p is written on success only.
  template <class T>
  int alloc(T** p, size_t count) {
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    mem.push_back(nullptr);                                 // room first: nothing can throw between hipMalloc and its record
    hipError_t e = hipMalloc(&mem.back(), bytes);
    if (e != hipSuccess) { mem.pop_back(); set_error("hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e)); return NNMPC_ENOMEM; }
    void* q = mem.back();
    e = hipMemset(q, 0, bytes);
    if (e != hipSuccess) { (void)give_back(q); set_error("hipMemset(%zu bytes): %s", bytes, hipGetErrorString(e)); return NNMPC_EHIP; }
    *p = (T*)q;
    return NNMPC_OK;
  }
  // alloc, then `count` elements from the host.
  template <class T>
  int upload(T** p, const T* src, size_t count) {
    T* q = nullptr;
    if (int rc = alloc(&q, count)) return rc;
    const hipError_t e = hipMemcpy(q, src, count * sizeof(T), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)give_back(q); set_error("hipMemcpy(%zu bytes to the device): %s", count * sizeof(T), hipGetErrorString(e)); return NNMPC_EHIP; }
    *p = q;
    return NNMPC_OK;
  }
  // Frees one buffer of alloc / upload before the handle dies (nullptr: nothing to do).
  int give_back(void* p) {
    if (!p) return NNMPC_OK;
    const auto it = std::find(mem.begin(), mem.end(), p);
    if (it == mem.end()) { set_error("give_back: %p is not a buffer of this handle", p); return NNMPC_EINVAL; }
    mem.erase(it);
    HIPCHK(hipFree(p));
    return NNMPC_OK;
  }

  // Slot i with room for `bytes`.  One growth rule; the old buffer goes before the new one is asked for, so the contents
  // are undefined after growth.
  static size_t grown(size_t bytes) { return bytes + bytes / 4 + 256; }
  template <class T>
  int slot(size_t i, T** out, size_t bytes) { return slot_of(slots, false, i, (void**)out, bytes); }
  template <class T>
  int pinned_slot(size_t i, T** out, size_t bytes) { return slot_of(pinned_slots, true, i, (void**)out, bytes); }
  int slot_of(std::vector<Slot>& v, bool pin, size_t i, void** out, size_t bytes) {
    if (i >= v.size()) { set_error("slot %zu of %zu", i, v.size()); return NNMPC_EINVAL; }
    Slot& s = v[i];
    if (s.cap < bytes) {
      if (s.p) { (void)(pin ? hipHostFree(s.p) : hipFree(s.p)); s = Slot{}; }
      const size_t want = grown(bytes);
      void* q = nullptr;
      const hipError_t e = pin ? hipHostMalloc(&q, want, hipHostMallocDefault) : hipMalloc(&q, want);
      if (e != hipSuccess) { set_error("%s(%zu bytes): %s", pin ? "hipHostMalloc" : "hipMalloc", want, hipGetErrorString(e)); return NNMPC_ENOMEM; }
      s = Slot{q, want};
    }
    *out = s.p;
    return NNMPC_OK;
  }

  // Frees slot i before the handle dies (its next use allocates again).  The caller has waited for whatever used it.
  void drop_slot(size_t i) {
    if (i < slots.size() && slots[i].p) { (void)hipFree(slots[i].p); slots[i] = Slot{}; }
  }

  // `count` elements of pinned host memory (default flags; not zeroed).
  template <class T>
  int pinned_alloc(T** p, size_t count) {
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    pinned.push_back(nullptr);
    const hipError_t e = hipHostMalloc(&pinned.back(), bytes, hipHostMallocDefault);
    if (e != hipSuccess) { pinned.pop_back(); set_error("hipHostMalloc(%zu bytes): %s", bytes, hipGetErrorString(e)); return NNMPC_ENOMEM; }
    *p = (T*)pinned.back();
    return NNMPC_OK;
  }

  int stream(hipStream_t* s) {
    streams.push_back(nullptr);
    const hipError_t e = hipStreamCreate(&streams.back());
    if (e != hipSuccess) { streams.pop_back(); set_error("hipStreamCreate: %s", hipGetErrorString(e)); return NNMPC_EHIP; }
    *s = streams.back();
    return NNMPC_OK;
  }
  int event(hipEvent_t* ev, unsigned flags = hipEventDefault) { return event_in(events, ev, flags); }
  // Event i of the pool, created as far as needed: stops at the first failure and holds created events only.
  int pool_event(size_t i, hipEvent_t* ev) {
    hipEvent_t last;
    while (pool.size() <= i)
      if (int rc = event_in(pool, &last, hipEventDefault)) return rc;
    *ev = pool[i];
    return NNMPC_OK;
  }
  int event_in(std::vector<hipEvent_t>& v, hipEvent_t* ev, unsigned flags) {
    v.push_back(nullptr);
    const hipError_t e = hipEventCreateWithFlags(&v.back(), flags);
    if (e != hipSuccess) { v.pop_back(); set_error("hipEventCreate: %s", hipGetErrorString(e)); return NNMPC_EHIP; }
    *ev = v.back();
    return NNMPC_OK;
  }

  // Waits for the device, then frees everything: events, device memory, pinned memory, streams.  Idempotent.
  void release() {
    if (mem.empty() && pinned.empty() && events.empty() && pool.empty() && streams.empty() &&
        std::none_of(slots.begin(), slots.end(), [](const Slot& s) { return s.p; }) &&
        std::none_of(pinned_slots.begin(), pinned_slots.end(), [](const Slot& s) { return s.p; })) return;
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    for (hipEvent_t e : pool) (void)hipEventDestroy(e);
    for (void* p : mem) (void)hipFree(p);
    for (Slot& s : slots) { if (s.p) (void)hipFree(s.p); s = Slot{}; }
    for (void* p : pinned) (void)hipHostFree(p);
    for (Slot& s : pinned_slots) { if (s.p) (void)hipHostFree(s.p); s = Slot{}; }
    for (hipStream_t s : streams) (void)hipStreamDestroy(s);
    events.clear(); pool.clear(); mem.clear(); pinned.clear(); streams.clear();
  }
};

// The arguments of a batched call whose caller hands host or device pointers (nnmpc.h, ptr_kind), one segment at a time:
// in() and out() give the device pointer of rows [r0, r0 + nr) of one argument with `per` elements a row.  A null argument
// gives a null pointer and no copy; a device pointer is offset; a host pointer gets slot `slot` of the owner (or `fixed`, a
// buffer the handle made at create), inputs copied in on the stream at once, outputs by copy_out() after the segment's
// kernels.  keep: the kernels need the output on the device whether or not the caller asked for it; it is not copied out
// unless asked for.  Slots grow only and a call's first segment is its largest, so no later segment moves a buffer.
struct Staging {
  DevRes& res; hipStream_t stream; bool host;
  struct Copy { void* dst; const void* src; size_t bytes; };
  Copy pending[8] = {};
  int npending = 0;

  template <class T>
  int in(const T** d, const T* p, size_t r0, size_t nr, size_t per, size_t slot, T* fixed = nullptr) {
    *d = nullptr;
    if (!p) return NNMPC_OK;
    if (!host) { *d = p + r0 * per; return NNMPC_OK; }
    const size_t bytes = nr * per * sizeof(T);
    T* q = fixed;
    if (!q) if (int rc = res.slot(slot, &q, std::max<size_t>(bytes, 1))) return rc;
    if (bytes) HIPCHK(hipMemcpyAsync(q, p + r0 * per, bytes, hipMemcpyHostToDevice, stream));
    *d = q;
    return NNMPC_OK;
  }
  template <class T>
  int out(T** d, T* p, size_t r0, size_t nr, size_t per, size_t slot, bool keep = false) {
    *d = nullptr;
    if (!p && !keep) return NNMPC_OK;
    if (!host && p) { *d = p + r0 * per; return NNMPC_OK; }
    const size_t bytes = nr * per * sizeof(T);
    if (p && npending == (int)(sizeof pending / sizeof pending[0])) { set_error("Staging: more than %d outputs", npending); return NNMPC_EINVAL; }
    if (int rc = res.slot(slot, d, std::max<size_t>(bytes, 1))) return rc;
    if (p && bytes) pending[npending++] = Copy{p + r0 * per, *d, bytes};
    return NNMPC_OK;
  }
  // Enqueues the segment's outputs for the caller; they are there once the stream has been waited for.
  int copy_out() {
    const int np = npending;
    npending = 0;
    for (int i = 0; i < np; ++i) HIPCHK(hipMemcpyAsync(pending[i].dst, pending[i].src, pending[i].bytes, hipMemcpyDeviceToHost, stream));
    return NNMPC_OK;
  }
};

// A handle under construction: `Destroy` (the handle's nnmpc_*_destroy) runs on every way out of create but the last
// line, which releases the handle into *out.
template <auto Destroy>
struct CallDestroy { template <class H> void operator()(H* h) const { Destroy(h); } };
template <class H, auto Destroy>
using Building = std::unique_ptr<H, CallDestroy<Destroy>>;

}  // namespace nnmpc
