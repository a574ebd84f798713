// csrc/launch.h -- the one way a kernel of libdsr_hip.so is launched, and the lists that pick a template instantiation (value_list.h).
#pragma once
#include "common.h"
#include "value_list.h"

namespace dsr {

// Dynamic LDS up to this size needs no opt-in; a launch that asks for more raises the kernel's limit first.  (0 would mean: whenever ldsBytes != 0.)
constexpr size_t kLdsOptInAbove = 64 * 1024;

// Launches kernel(args...) and throws on a launch the runtime refuses, so the error names this launch and not a later one.  The arguments are
// converted to the kernel's parameter types here; a cast that changes what a pointer points to, (const float2*) X, is the caller's.
template <class... P, class... A>
void launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t ldsBytes, hipStream_t st, A&&... args)
{
  static_assert(sizeof...(P) == sizeof...(A), "launch: argument count differs from the kernel's parameter count");
  if (ldsBytes > kLdsOptInAbove) DSR_HIP(hipFuncSetAttribute((const void*) kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) ldsBytes));
  hipLaunchKernelGGL(kernel, grid, block, ldsBytes, st, static_cast<P>(args)...);
  DSR_HIP(hipGetLastError());
}

}  // namespace dsr
