// How a chosen kernel is launched (host side): the dynamic-LDS launch, the dtype dispatch, the per-stream scratch and the
// "slabs -> launch -> ordered fold" sequence of the weight-gradient kernels.  Which kernel is chosen: conv_route.cpp and the families.
#pragma once
#include <atomic>

#include "common.hpp"

namespace sslcr {

int device_cus();      // compute units of the current device (asked once per process, thread-safely; 256 if the query fails)

// per-stream scratch for partial results that a follow-up launch on the SAME stream folds in a fixed order: the accumulator slabs of
// the weight-gradient kernels (wgrad_fold_kernel) and the per-workgroup rows of the BatchNorm-backward reduce pass (bn_bwd_sums_kernel)
void* stream_scratch(hipStream_t st, size_t bytes);
void stream_scratch_release();      // frees every stream's scratch (sslcr_destroy, after a device synchronise)
// the launches that fold the slabs, wgrad_halo.hip
hipError_t launch_wgrad_fold(const void* slabs, float* dw, int C, int gx, int gy, int splits, int taps, int kh_n, hipStream_t st);
hipError_t launch_stem_wgrad_fold(const void* slabs, float* dw, int nwg, hipStream_t st);

// Launch Kern with `lds` bytes of dynamic LDS, of which the kernel may ask up to `cap`.  The limit is raised once per template
// instance (Kern and its argument types) and per PROCESS, not per device: a process drives one device.
template <auto Kern, class... A>
hipError_t launch_lds(dim3 grid, dim3 block, size_t lds, size_t cap, hipStream_t st, A... args) {
  if (lds > cap) return hipErrorInvalidValue;
  static std::atomic<bool> raised{false};
  if (!raised) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)cap);
    if (e != hipSuccess) return e;
    raised = true;
  }
  hipLaunchKernelGGL(Kern, grid, block, lds, st, args...);
  return hipGetLastError();
}

// f(bf16_t{}) or f(float{}): one launch line for both element types
template <class F>
auto by_dtype(int dtype, F&& f) { return dtype == DT_BF16 ? f(bf16_t{}) : f(float{}); }

// The split launches of the weight-gradient kernels: more than one split -> accumulator slabs from the stream's scratch, launch(slabs),
// fold(slabs) in a fixed order; a single split launches with slabs == nullptr and folds nothing.  No scratch is an error -- there is
// no atomic path to fall back to: its summation order would differ.
template <class L, class F>
hipError_t with_slabs(hipStream_t st, size_t bytes_if_split, L&& launch, F&& fold) {
  f32x4_t* slabs = nullptr;
  if (bytes_if_split) {
    slabs = reinterpret_cast<f32x4_t*>(stream_scratch(st, bytes_if_split));
    if (!slabs) return hipErrorOutOfMemory;
  }
  const hipError_t e = launch(slabs);
  return slabs && e == hipSuccess ? fold(slabs) : e;
}

}  // namespace sslcr
