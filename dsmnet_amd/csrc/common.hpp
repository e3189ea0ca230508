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

// One output pixel of utils/imwrap.py:37-72 imwrap_BCHW (fliplr False, LeftTop [0,0], scale 1) as this
// torch's grid_sample(bilinear, zeros, align_corners=False) evaluates it -- shared by warp.hip and
// metrics.hip so that both sample the very same value.  (x, y) is the pixel of the (H, W) disparity map, d
// its disparity, (H0, W0) the sampled image, x1 / y1 the last point of the base grid (linspace(-1, x1, W)).
// |ix| can be huge for wild disparities: clamp before the int conversion (both taps then fall outside and
// contribute zero, as in torch).
struct dsm_warp_taps {
  int x0, y0;                    // the nw tap; dereference behind i00..i11 only
  float wx0, wx1, wy0, wy1;
  float nw, ne, sw, se;
  bool i00, i01, i10, i11;       // tap in bounds: nw, ne, sw, se
};

__device__ __forceinline__ dsm_warp_taps dsm_warp_taps_at(float d, int x, int y, int H, int W, int H0,
                                                          int W0, float x1, float y1) {
  dsm_warp_taps t;
  const float gx = linspace_at(-1.f, x1, W, x) - d * 2.0f / (float)(W0 - 1);
  const float gy = linspace_at(-1.f, y1, H, y);
  const float ix = ((gx + 1.f) * (float)W0 - 1.f) / 2.f;
  const float iy = ((gy + 1.f) * (float)H0 - 1.f) / 2.f;
  const float fx = floorf(ix), fy = floorf(iy);
  t.x0 = (int)fminf(fmaxf(fx, -2.f), (float)W0 + 1.f);
  t.y0 = (int)fminf(fmaxf(fy, -2.f), (float)H0 + 1.f);
  t.wx1 = ix - fx; t.wx0 = (fx + 1.f) - ix; t.wy1 = iy - fy; t.wy0 = (fy + 1.f) - iy;
  const bool inx0 = t.x0 >= 0 && t.x0 < W0, inx1 = t.x0 + 1 >= 0 && t.x0 + 1 < W0;
  const bool iny0 = t.y0 >= 0 && t.y0 < H0, iny1 = t.y0 + 1 >= 0 && t.y0 + 1 < H0;
  t.i00 = iny0 && inx0; t.i01 = iny0 && inx1; t.i10 = iny1 && inx0; t.i11 = iny1 && inx1;
  t.nw = t.wx0 * t.wy0; t.ne = t.wx1 * t.wy0; t.sw = t.wx0 * t.wy1; t.se = t.wx1 * t.wy1;
  return t;
}

// the sample itself: taps in the order nw, ne, sw, se, the reference's `+ delt` on in-bounds taps only
// (out-of-bounds taps of `im_src + delt` are zeros)
__device__ __forceinline__ float dsm_warp_sample(const dsm_warp_taps& t, float v00, float v01, float v10,
                                                 float v11, float delt) {
  float v = 0.f;
  if (t.i00) v += (v00 + delt) * t.nw;
  if (t.i01) v += (v01 + delt) * t.ne;
  if (t.i10) v += (v10 + delt) * t.sw;
  if (t.i11) v += (v11 + delt) * t.se;
  return v;
}

// sum over the wave's 64 lanes, in every lane (xor butterfly)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
