// Stereo spatial augmentation of a training batch in one pass:
//   myTransforms/aug_spatial.py:7-88   Spatial_stereo: random shift of the right view, random crop,
//                                      optional random scale (cv2.resize, linear)
//   myTransforms/aug_color.py:15-26    ToTensor_numpy: HWC -> CHW, first `channel` planes / 255
// The reference runs these per frame on the host with numpy and cv2.  Here the host draws every
// random number (in the reference's order) into one record per image that travels in the kernel
// arguments, and one launch turns the (B, H0, W0, C) frames into the (B, C, h, w) batch.
//
// Memory-bound: a thread takes one output pixel.  Per tap it reads the pixel's C contiguous floats
// (channels 3..5 and 7 from the pixel `shift` columns to the right), neighbouring threads read
// neighbouring pixels, and every channel plane is written with consecutive lanes on consecutive
// floats.  Crop only: 4C B read + 4C B written per output pixel.  Resize: the four taps of
// neighbouring outputs overlap, so HBM sees each source pixel of the window once.
//
// Arithmetic is the reference's fp32 sequence with no contraction (the pragma below): the masked
// `+ shift` on channels >= 6 on every tap, horizontal lerp S[sx]*(1-fx) + S[sx+1]*fx, vertical
// lerp of the two row results, `* scale_rand` on channels >= 6, `/ 255` on the first
// `to_tensor_channels`.  The tap coordinate is formed in fp64 and cast to fp32, as cv2 does.
#include <math.h>
#include <string.h>

#include "common.hpp"
#include "spatial_taps.hpp"

#pragma clang fp contract(off)

namespace {

struct SpatialRecords {
  dsm_spatial_record r[DSM_SPATIAL_MAX_RECORDS];
};

// Work item = (image of the chunk, output row, output column); grid-stride over nb * h * w items.
// C is a template parameter so that the channel loops unroll and every load of a pixel is in flight
// before the first is used.
template <int C>
__global__ __launch_bounds__(256) void stereo_spatial_kernel(const float* __restrict__ x,
                                                             float* __restrict__ y, SpatialRecords recs,
                                                             int b0, int nb, int H0, int W0,
                                                             int h, int w, int to_tensor) {
  const unsigned total = (unsigned)nb * (unsigned)h * (unsigned)w;
  const size_t in_image = (size_t)H0 * W0 * C, plane = (size_t)h * w;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const unsigned row = i / (unsigned)w, ox = i - row * (unsigned)w;
    const unsigned bl = row / (unsigned)h, oy = row - bl * (unsigned)h;
    const dsm_spatial_record& rec = recs.r[bl];
    const float* src = x + (size_t)(b0 + (int)bl) * in_image;
    float* dst = y + (size_t)(b0 + (int)bl) * C * plane + (size_t)oy * w + ox;
    const int shift = rec.shift;
    const float fshift = (float)shift;
    if (!rec.resize) {                            // pure gather (the window is h x w)
      const int p = ((rec.hs + (int)oy) * W0 + rec.ws + (int)ox) * C;
      float v[C];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        v[c] = src[p + (spatial_right_channel(c) ? shift * C : 0) + c];
      }
#pragma unroll
      for (int c = 0; c < C; ++c)
        dst[(size_t)c * plane] = spatial_finish_crop(v[c], c, fshift, to_tensor);
      continue;
    }
    int sx, sy;
    float fx, fy;
    resize_tap((int)ox, rec.scale_x, rec.w, sx, fx);
    resize_tap((int)oy, rec.scale_y, rec.h, sy, fy);
    const int sx1 = min(sx + 1, rec.w - 1), sy1 = min(sy + 1, rec.h - 1);
    const int r0 = (rec.hs + sy) * W0, r1 = (rec.hs + sy1) * W0;
    const int c0 = rec.ws + sx, c1 = rec.ws + sx1;
    const float gx = 1.f - fx, gy = 1.f - fy;
    float t[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int o = (spatial_right_channel(c) ? shift * C : 0) + c;
      t[c][0] = src[(r0 + c0) * C + o];
      t[c][1] = src[(r0 + c1) * C + o];
      t[c][2] = src[(r1 + c0) * C + o];
      t[c][3] = src[(r1 + c1) * C + o];
    }
#pragma unroll
    for (int c = 0; c < C; ++c)
      dst[(size_t)c * plane] = spatial_finish_resize(t[c][0], t[c][1], t[c][2], t[c][3], c, fshift, gx, fx, gy, fy,
                                                     rec.scale_rand, to_tensor);
  }
}

}  // namespace

extern "C" int dsm_stereo_spatial(const void* x, void* y, const dsm_spatial_record* recs, int n_recs,
                                  int B, int C, int H0, int W0, int h, int w, int to_tensor_channels,
                                  dsm_stream_t stream) {
  DSM_REQUIRE(x && y && recs, DSM_ERR_ARG);
  DSM_REQUIRE(B > 0 && H0 > 0 && W0 > 0 && h > 0 && w > 0, DSM_ERR_ARG);
  DSM_REQUIRE(C >= 6 && C <= 8, DSM_ERR_ARG);
  DSM_REQUIRE(n_recs == B, DSM_ERR_ARG);
  DSM_REQUIRE(to_tensor_channels == 0 || to_tensor_channels == 6, DSM_ERR_ARG);
  for (int i = 0; i < n_recs; ++i) DSM_REQUIRE(spatial_record_ok(recs[i], H0, W0, h, w), DSM_ERR_ARG);
  DSM_REQUIRE((long)H0 * W0 * C < (1L << 31) && (long)h * w * C < (1L << 31), DSM_ERR_UNSUPPORTED);
  DSM_REQUIRE(((uintptr_t)x & 3u) == 0 && ((uintptr_t)y & 3u) == 0, DSM_ERR_ALIGN);
  const long per_image = (long)h * w;
  long chunk = DSM_SPATIAL_MAX_RECORDS;
  if (chunk * per_image >= (1L << 31)) chunk = ((1L << 31) - 1) / per_image;   // 32-bit work-item index
  dsm_clear_stale_error();
  for (int b0 = 0; b0 < B; b0 += (int)chunk) {
    const int nb = (int)(B - b0 < chunk ? B - b0 : chunk);
    SpatialRecords r;
    ::memset(&r, 0, sizeof(r));
    ::memcpy(r.r, recs + b0, sizeof(dsm_spatial_record) * (size_t)nb);
    const int blocks = dsm_cdiv((long)nb * per_image, 256);
    const int grid = blocks < 4096 ? blocks : 4096;
    auto kernel = C == 6 ? stereo_spatial_kernel<6> : C == 7 ? stereo_spatial_kernel<7> : stereo_spatial_kernel<8>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream,
                       (const float*)x, (float*)y, r, b0, nb, H0, W0, h, w, to_tensor_channels);
    const int st = dsm_launch_status();
    if (st != DSM_OK) return st;
  }
  return DSM_OK;
}
