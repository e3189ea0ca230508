// The arithmetic that spatial.hip (fp32 frames) and frames.hip (raw 8/16-bit planes) share, so that
// the two kernels cannot drift: cv2's linear-resize tap, which channels read
// the shifted column, the per-channel finish of a crop and of a resize pixel, and the host check of
// one record.  Everything here is the reference's fp32 sequence with no contraction.
#pragma once
#include <math.h>

#include "common.hpp"

// No contraction from here to the end of the including file: the fp64 tap coordinate and the fp32
// lerps are the reference's sequence of separately rounded operations.
#pragma clang fp contract(off)

// channels 3..5 (imR) and 7 (dispR) are read `shift` columns to the right (aug_spatial.py:17-41)
__host__ __device__ __forceinline__ constexpr bool spatial_right_channel(int c) {
  return (c >= 3 && c < 6) || c == 7;
}

// cv2's linear-resize coordinate of output index d: tap s in [0, n), weight f of tap min(s+1, n-1)
__device__ __forceinline__ void resize_tap(int d, double scale, int n, int& s, float& f) {
  f = (float)(((double)d + 0.5) * scale - 0.5);
  const float fl = floorf(f);
  s = (int)fl;
  f -= fl;
  if (s < 0) { s = 0; f = 0.f; }
  if (s >= n - 1) { s = n - 1; f = 0.f; }
}

// crop only: the masked `+ shift` on channels >= 6, `/ 255` on the first `to_tensor`
__device__ __forceinline__ float spatial_finish_crop(float v, int c, float fshift, int to_tensor) {
  if (c >= 6 && v != 0.f) v += fshift;
  if (c < to_tensor) v = v / 255.0f;
  return v;
}

// resize: the masked `+ shift` on every tap, the horizontal then the vertical lerp, `* scale_rand`
// on channels >= 6, `/ 255` on the first `to_tensor`
__device__ __forceinline__ float spatial_finish_resize(float t00, float t01, float t10, float t11, int c,
                                                       float fshift, float gx, float fx, float gy, float fy,
                                                       float scale_rand, int to_tensor) {
  if (c >= 6) {
    if (t00 != 0.f) t00 += fshift;
    if (t01 != 0.f) t01 += fshift;
    if (t10 != 0.f) t10 += fshift;
    if (t11 != 0.f) t11 += fshift;
  }
  const float a = t00 * gx + t01 * fx;
  const float b = t10 * gx + t11 * fx;
  float v = a * gy + b * fy;
  if (c >= 6) v = v * scale_rand;
  if (c < to_tensor) v = v / 255.0f;
  return v;
}

static inline bool spatial_record_ok(const dsm_spatial_record& r, int H0, int W0, int h, int w) {
  if (r.shift < 0 || r.shift >= W0) return false;
  if (r.w < 1 || r.h < 1 || r.ws < 0 || r.hs < 0) return false;
  if ((long)r.ws + r.w > (long)W0 - r.shift || (long)r.hs + r.h > (long)H0) return false;
  if (r.resize != 0 && r.resize != 1) return false;
  if (!r.resize) return r.w == w && r.h == h;
  return isfinite(r.scale_x) && isfinite(r.scale_y) && r.scale_x > 0 && r.scale_y > 0 &&
         isfinite(r.scale_rand);
}
