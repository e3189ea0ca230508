// Stereo colour augmentation of a training batch in one pass:
//   myTransforms/__init__.py:109-135  Stereo_color / Stereo_normalize through Stereo_color_batch
//   myTransforms/aug_color.py:175-203 RandomOrder over Brightness / Contrast / Saturation / Gamma
//                                     (:103-173), then clamp(0, 1)
//   myTransforms/aug_color.py:66-101  Lighting (ImageNet PCA noise), clamp(0, 1)
//   myTransforms/aug_color.py:28-45   Normalize (ImageNet mean / std)
// The reference runs these per image with ~100 small launches each; here the host draws every
// random number (in the reference's order) into per-(image, group) records that travel in the
// kernel arguments, Lighting's alpha stays on the device, and one launch rewrites the batch in place.
//
// Memory-bound: 24 B read + 24 B written per pixel for the two RGB groups.  A thread takes 4
// consecutive pixels of a row and all channels of every group: float4 loads / stores when the row
// length allows (W % 4 == 0, 16-byte aligned base), a predicated scalar quad otherwise.
// Arithmetic follows the reference's fp32 sequence: the scalars arrive as the reference applies
// them (1 + u for Brightness and Gamma), the grey is 0.299 R + 0.587 G + 0.114 B of the current
// values, clamps keep NaN as torch.clamp does, Normalize divides.  Drift: Gamma clamps its base at
// 0 (the reference's negative ** non-integer is NaN).
#include <string.h>

#include "common.hpp"

namespace {

struct ColorRecords {
  dsm_color_record r[DSM_COLOR_MAX_RECORDS];
};

// myTransforms/aug_color.py:7-13 (imagenet_pca) and __init__.py:8 (__imagenet_normalize)
__device__ constexpr float kEigval[3] = {0.2175f, 0.0188f, 0.0045f};
__device__ constexpr float kEigvec[3][3] = {{-0.5675f, 0.7192f, 0.4009f},
                                            {-0.5808f, -0.0045f, -0.8140f},
                                            {-0.5836f, -0.6948f, 0.4203f}};
__device__ constexpr float kMean[3] = {0.485f, 0.456f, 0.406f};
__device__ constexpr float kStd[3] = {0.229f, 0.224f, 0.225f};

// torch.clamp(0, 1): NaN stays NaN (both comparisons are false)
__device__ __forceinline__ float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

// One group (3 channels) of 4 pixels, v[channel][pixel], through the record's steps.
__device__ __forceinline__ void color_group(float (&v)[3][4], const dsm_color_record& rec,
                                            const float* __restrict__ alpha) {
  const int flags = rec.flags;
  if (flags & DSM_COLOR_JITTER) {
#pragma unroll 1                                 // one copy of each step's code (powf is long)
    for (int k = 0; k < 4; ++k) {
      const int t = rec.order[k];
      const float j = rec.jitter[t];
      if (t == 0) {                              // Brightness: x * (1 + u)
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int e = 0; e < 4; ++e) v[c][e] = v[c][e] * j;
      } else if (t == 1) {                       // Contrast: x + u
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int e = 0; e < 4; ++e) v[c][e] = v[c][e] + j;
      } else if (t == 2) {                       // Saturation: x + gray * u (gray before the step)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float gray = v[0][e] * 0.299f + 0.587f * v[1][e] + 0.114f * v[2][e];
#pragma unroll
          for (int c = 0; c < 3; ++c) v[c][e] = v[c][e] + gray * j;
        }
      } else {                                   // Gamma: max(x, 0) ** (1 + u), accurate powf
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int e = 0; e < 4; ++e) v[c][e] = powf(v[c][e] < 0.f ? 0.f : v[c][e], j);
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[c][e] = clamp01(v[c][e]);
  }
  if (flags & DSM_COLOR_LIGHTING) {
    const float* a = alpha + 3 * (size_t)rec.alpha_row;
    const float a0 = a[0], a1 = a[1], a2 = a[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float rgb = kEigvec[c][0] * a0 * kEigval[0] + kEigvec[c][1] * a1 * kEigval[1] +
                        kEigvec[c][2] * a2 * kEigval[2];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[c][e] = clamp01(v[c][e] + rgb);
    }
  }
  if (flags & DSM_COLOR_NORMALIZE) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[c][e] = (v[c][e] - kMean[c]) / kStd[c];
  }
}

// Work item = (image of the chunk, row, quad of 4 pixels); grid-stride over nb * H * Q items.
template <bool VEC>
__global__ __launch_bounds__(256) void stereo_color_kernel(float* __restrict__ x,
                                                           const float* __restrict__ alpha,
                                                           ColorRecords recs, int b0, int nb, int C,
                                                           int H, int W, int groups, int Q) {
  const unsigned total = (unsigned)nb * (unsigned)H * (unsigned)Q;
  const size_t plane = (size_t)H * W;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const unsigned row = i / (unsigned)Q, q = i - row * (unsigned)Q;
    const unsigned bl = row / (unsigned)H, y = row - bl * (unsigned)H;
    const int x0 = 4 * (int)q;
    const int n = VEC ? 4 : min(4, W - x0);
    float* base = x + ((size_t)(b0 + (int)bl) * C) * plane + (size_t)y * W + x0;
    for (int g = 0; g < groups; ++g) {
      float* p = base + (size_t)(3 * g) * plane;
      float v[3][4];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (VEC) {
          const f32x4 t = *reinterpret_cast<const f32x4*>(p + c * plane);
          v[c][0] = t.x; v[c][1] = t.y; v[c][2] = t.z; v[c][3] = t.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[c][e] = e < n ? p[c * plane + e] : 0.f;
        }
      }
      color_group(v, recs.r[bl * groups + g], alpha);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (VEC) {
          f32x4 t;
          t.x = v[c][0]; t.y = v[c][1]; t.z = v[c][2]; t.w = v[c][3];
          *reinterpret_cast<f32x4*>(p + c * plane) = t;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (e < n) p[c * plane + e] = v[c][e];
        }
      }
    }
  }
}

bool color_record_ok(const dsm_color_record& r, int n_recs, const void* alpha) {
  if (r.flags & ~(DSM_COLOR_JITTER | DSM_COLOR_LIGHTING | DSM_COLOR_NORMALIZE)) return false;
  int seen = 0;
  for (int k = 0; k < 4; ++k) {
    if (r.order[k] < 0 || r.order[k] > 3) return false;
    seen |= 1 << r.order[k];
  }
  if (seen != 15) return false;
  if (r.flags & DSM_COLOR_LIGHTING) return alpha != nullptr && r.alpha_row >= 0 && r.alpha_row < n_recs;
  return true;
}

}  // namespace

extern "C" int dsm_stereo_color(void* x, const void* alpha, const dsm_color_record* recs, int n_recs,
                                int B, int C, int H, int W, int groups, dsm_stream_t stream) {
  DSM_REQUIRE(x && recs, DSM_ERR_ARG);
  DSM_REQUIRE(B > 0 && C >= 6 && H > 0 && W > 0, DSM_ERR_ARG);
  DSM_REQUIRE(groups == 1 || groups == 2, DSM_ERR_ARG);
  DSM_REQUIRE((long)B * groups == (long)n_recs, DSM_ERR_ARG);
  for (int i = 0; i < n_recs; ++i) DSM_REQUIRE(color_record_ok(recs[i], n_recs, alpha), DSM_ERR_ARG);
  const long Q = (W + 3) / 4;
  const long per_image = (long)H * Q;
  DSM_REQUIRE(per_image < (1L << 31), DSM_ERR_UNSUPPORTED);     // 32-bit work-item index
  long chunk = DSM_COLOR_MAX_RECORDS / groups;
  if (chunk * per_image >= (1L << 31)) chunk = ((1L << 31) - 1) / per_image;
  const bool vec = (W % 4 == 0) && dsm_aligned16(x);
  dsm_clear_stale_error();
  for (int b0 = 0; b0 < B; b0 += (int)chunk) {
    const int nb = (int)(B - b0 < chunk ? B - b0 : chunk);
    ColorRecords r;
    ::memset(&r, 0, sizeof(r));
    ::memcpy(r.r, recs + (size_t)b0 * groups, sizeof(dsm_color_record) * (size_t)nb * groups);
    const int grid = (int)(dsm_cdiv((long)nb * per_image, 256) < 2048 ? dsm_cdiv((long)nb * per_image, 256) : 2048);
    if (vec)
      hipLaunchKernelGGL(stereo_color_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream,
                         (float*)x, (const float*)alpha, r, b0, nb, C, H, W, groups, (int)Q);
    else
      hipLaunchKernelGGL(stereo_color_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream,
                         (float*)x, (const float*)alpha, r, b0, nb, C, H, W, groups, (int)Q);
    const int st = dsm_launch_status();
    if (st != DSM_OK) return st;
  }
  return DSM_OK;
}
