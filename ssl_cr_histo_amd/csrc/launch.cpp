// Host utilities of the launch layer (launch.hpp): the device's compute-unit count and the per-stream scratch.
#include <cstdio>
#include <mutex>

#include "kernels.hpp"

namespace sslcr {

int device_cus() {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    return n;
  }();
  return cus;
}

// slabs of the launches on one stream (a launch's fold has consumed them before the next launch on that stream writes; the
// BatchNorm-backward reduce pass keeps its per-workgroup rows here too).
// One entry per stream, 64 entries, least-recently-used eviction (logged once: it costs a device synchronise): a 65th stream (virtual-rank tests create a stream per context
// and drop it) takes over the oldest entry after a device synchronise -- never a silent fall-back to the atomic path, whose
// summation order differs -- and an evicted or destroyed stream's slab is freed instead of leaking.
namespace {
struct Slab { hipStream_t st; void* p; size_t cap; unsigned long long used; };
constexpr int NSLAB = 64;
Slab g_slabs[NSLAB];
int g_nslabs = 0;
unsigned long long g_slab_tick = 0;
std::mutex g_slab_mu;                            // host threads driving different streams
}  // namespace
// sslcr_destroy: every stream's slab is freed (the device has been synchronised; a later launch allocates again)
void stream_scratch_release() {
  std::lock_guard<std::mutex> lock(g_slab_mu);
  for (int i = 0; i < g_nslabs; ++i)
    if (g_slabs[i].p) (void)hipFree(g_slabs[i].p);
  g_nslabs = 0;
}
void* stream_scratch(hipStream_t st, size_t bytes) {
  Slab* const slabs = g_slabs;
  int& n = g_nslabs;
  unsigned long long& tick = g_slab_tick;
  std::lock_guard<std::mutex> lock(g_slab_mu);
  Slab* e = nullptr;
  for (int i = 0; i < n && !e; ++i)
    if (slabs[i].st == st) e = &slabs[i];
  if (!e) {
    if (n < NSLAB) {
      e = &slabs[n++];
    } else {
      e = &slabs[0];
      for (int i = 1; i < NSLAB; ++i)
        if (slabs[i].used < e->used) e = &slabs[i];
      static bool warned = false;
      if (!warned) {
        warned = true;
        fprintf(stderr, "sslcr: more than %d streams have launched weight-gradient / BatchNorm-backward kernels; the least recently used "
                        "stream's slab is evicted after a device synchronise (slow when it happens per launch)\n", NSLAB);
      }
      (void)hipDeviceSynchronize();              // the evicted stream may be gone: wait for the device, not for the stream
      if (e->p) (void)hipFree(e->p);
    }
    *e = Slab{st, nullptr, 0, 0};
  }
  e->used = ++tick;
  if (e->cap < bytes) {
    if (e->p) {
      (void)hipStreamSynchronize(st);
      (void)hipFree(e->p);
    }
    e->p = nullptr; e->cap = 0;
    if (hipMalloc(&e->p, bytes) != hipSuccess) return nullptr;
    e->cap = bytes;
  }
  return e->p;
}

}  // namespace sslcr
