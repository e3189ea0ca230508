// Shared helpers for the gfx950 kernels of the stereo cost-volume path.
// Written for CDNA4 only: wave = 64 lanes, 256 CUs in 8 XCDs, 160 KiB LDS per CU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "../../include/dsmnet_hip.h"

#define DSM_WAVE 64

// ext-vector float4 with 4-byte alignment: gfx950 global/LDS dwordx4 accesses
// only need dword alignment, so shifted (x - d) rows can still move 16 B per lane.
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// hipGetLastError() is sticky per thread and is shared with everything else in the
// process (PyTorch, MIOpen ...): drop whatever an earlier, unrelated call left behind
// before launching, so that dsm_launch_status() reports only this library's launch.
static inline void dsm_clear_stale_error() { (void)hipGetLastError(); }

static inline int dsm_launch_status() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? DSM_OK : DSM_ERR_LAUNCH;
}

static inline bool dsm_aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }

static inline int dsm_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

#define DSM_REQUIRE(cond, code) do { if (!(cond)) return (code); } while (0)

// Make sure `kernel` may use `bytes` of dynamic LDS (past 64 KiB a kernel's limit has to be raised before
// its first launch).  The flag -- one per kernel and host thread -- is the only state the library keeps
// (DESIGN.md 1): a launch after the first pays one thread-local load.  Only the FIRST call's `bytes` reaches
// the runtime, and nothing here checks later ones against it: every caller passes a size that is fixed per
// kernel instantiation (a compile-time constant, or the most any of its plans may ask for).
template <auto kernel>
static inline int dsm_allow_lds(size_t bytes) {
  static thread_local bool configured = false;
  if (!configured) {
    if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
      return DSM_ERR_LAUNCH;
    configured = true;
  }
  return DSM_OK;
}

// torch.linspace(start, end, steps)[i], evaluated as torch does (from the nearer end)
__device__ __forceinline__ float linspace_at(float start, float end, int steps, int i) {
  const float step = (end - start) / (float)(steps - 1);
  return i < steps / 2 ? start + step * (float)i : end - step * (float)(steps - i - 1);
}

// sum over the wave's 64 lanes, in every lane (xor butterfly)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
