// From the decoded files' bytes to the training batch in one pass:
//   myDatasets_stereo/Dataset_stereo.py:63-74    Crop_center_bottom to the common size
//   myDatasets_stereo/Dataset_stereo.py:86-99    np.float32 and the channel concatenation
//   myDatasets_stereo/Dataset_stereo.py:121-123  the random horizontal flip (views are not swapped)
// followed by what spatial.hip does (aug_spatial.py:7-88, aug_color.py:15-26).  The reference forms
// the (H0, W0, C) fp32 frame on the host; here it is never formed.  Every sample's planes lie in one
// byte buffer as they were decoded -- (Hs, Ws, 3) uint8 RGB, (Hs, Ws) uint8 / uint16 / float32
// disparity -- and a dsm_frame_source per image says where, which H0 x W0 window of them is the
// frame, and whether it is mirrored.  Frame pixel (y, x) is source pixel
// (y0 + y, x0 + (flip ? W0 - 1 - x : x)); from there on the kernel is spatial.hip's: same records,
// same taps, same float sequence (spatial_taps.hpp), so the batch is bit-identical to assembling the
// fp32 frames and calling dsm_stereo_spatial (uint8 -> float and uint16 / 256 are exact).
//
// Memory-bound: a thread takes one output pixel, neighbouring threads read neighbouring source
// pixels (mirrored: in descending order, the same cache lines), and every channel plane is written
// with consecutive lanes on consecutive floats.  Crop only: 6..14 B read + 4C B written per output
// pixel.  A pixel's RGB bytes are loaded before the disparity format is looked at, and each format's
// taps are loaded together, so all of a pixel's loads are in flight before the first is used.
// Sources and records travel in kernel arguments (112 B per image).  Every plane is bounds-checked
// against raw_bytes on the host before a launch, so the kernel cannot read outside `raw`.
#include <math.h>
#include <string.h>

#include "common.hpp"
#include "spatial_taps.hpp"

#pragma clang fp contract(off)

namespace {

struct FrameArgs {
  dsm_spatial_record r[DSM_FRAMES_MAX_RECORDS];
  dsm_frame_source s[DSM_FRAMES_MAX_RECORDS];
};
static_assert(sizeof(dsm_frame_source) == 64, "dsm_frame_source is 64 bytes");
static_assert(sizeof(FrameArgs) == 112 * DSM_FRAMES_MAX_RECORDS, "112 B per image");

// element `idx` of a disparity plane at byte offset `off` of raw, as the float the host would form
__device__ __forceinline__ float disp_at(const unsigned char* __restrict__ raw, long long off, int format,
                                         int idx) {
  const unsigned char* p = raw + off;
  switch (format) {
    case DSM_DISP_F32: {
      const float v = ((const float*)p)[idx];
      return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u ? 0.f : v;   // inf, nan -> 0
    }
    case DSM_DISP_U16_256: return (float)((const unsigned short*)p)[idx] / 256.0f;
    case DSM_DISP_U16: return (float)((const unsigned short*)p)[idx];
    default: return (float)p[idx];
  }
}

// The C channels of source pixels (row, colL) and, for the shifted channels, (row, colR)
template <int C>
__device__ __forceinline__ void load_pixel(const unsigned char* __restrict__ raw, const dsm_frame_source& s,
                                           int row, int colL, int colR, float* v) {
  const int iL = row * s.Ws + colL, iR = row * s.Ws + colR;
  const unsigned char* pl = raw + s.imL + (size_t)iL * 3;
  const unsigned char* pr = raw + s.imR + (size_t)iR * 3;
  const unsigned char l0 = pl[0], l1 = pl[1], l2 = pl[2], r0 = pr[0], r1 = pr[1], r2 = pr[2];
  if (C >= 7) v[6] = disp_at(raw, s.dispL, s.disp_format, iL);
  if (C >= 8) v[7] = disp_at(raw, s.dispR, s.disp_format, iR);
  v[0] = (float)l0; v[1] = (float)l1; v[2] = (float)l2;
  v[3] = (float)r0; v[4] = (float)r1; v[5] = (float)r2;
}

// Work item = (image of the chunk, output row, output column); grid-stride over nb * h * w items.
template <int C>
__global__ __launch_bounds__(256) void stereo_spatial_raw_kernel(const unsigned char* __restrict__ raw,
                                                                 float* __restrict__ y, FrameArgs a, int b0,
                                                                 int nb, int W0, int h, int w, int to_tensor) {
  const unsigned total = (unsigned)nb * (unsigned)h * (unsigned)w;
  const size_t plane = (size_t)h * w;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const unsigned row = i / (unsigned)w, ox = i - row * (unsigned)w;
    const unsigned bl = row / (unsigned)h, oy = row - bl * (unsigned)h;
    const dsm_spatial_record& rec = a.r[bl];
    const dsm_frame_source& s = a.s[bl];
    float* dst = y + (size_t)(b0 + (int)bl) * C * plane + (size_t)oy * w + ox;
    const int shift = rec.shift;
    const float fshift = (float)shift;
    // frame column x -> source column: x0 + x, or mirrored x0 + W0 - 1 - x
    const int xbase = s.flip ? s.x0 + W0 - 1 : s.x0, xstep = s.flip ? -1 : 1;
    if (!rec.resize) {                            // pure gather (the window is h x w)
      const int fx0 = rec.ws + (int)ox;
      float v[C];
      load_pixel<C>(raw, s, s.y0 + rec.hs + (int)oy, xbase + xstep * fx0, xbase + xstep * (fx0 + shift), v);
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
    const int r0 = s.y0 + rec.hs + sy, r1 = s.y0 + rec.hs + sy1;
    const int c0 = rec.ws + sx, c1 = rec.ws + sx1;
    const int c0L = xbase + xstep * c0, c0R = xbase + xstep * (c0 + shift);
    const int c1L = xbase + xstep * c1, c1R = xbase + xstep * (c1 + shift);
    const float gx = 1.f - fx, gy = 1.f - fy;
    float t00[C], t01[C], t10[C], t11[C];
    load_pixel<C>(raw, s, r0, c0L, c0R, t00);
    load_pixel<C>(raw, s, r0, c1L, c1R, t01);
    load_pixel<C>(raw, s, r1, c0L, c0R, t10);
    load_pixel<C>(raw, s, r1, c1L, c1R, t11);
#pragma unroll
    for (int c = 0; c < C; ++c)
      dst[(size_t)c * plane] = spatial_finish_resize(t00[c], t01[c], t10[c], t11[c], c, fshift, gx, fx, gy, fy,
                                                     rec.scale_rand, to_tensor);
  }
}

// [off, off + Hs * Ws * elem) inside [0, raw_bytes)?  The product cannot overflow: Hs, Ws < 2^31, elem <= 4.
bool plane_inside(long long off, int Hs, int Ws, int elem, size_t raw_bytes) {
  if (off < 0 || (unsigned long long)off > raw_bytes) return false;
  const unsigned long long bytes = (unsigned long long)Hs * (unsigned long long)Ws * (unsigned)elem;
  return bytes <= raw_bytes - (unsigned long long)off;
}

// px * bytes_per_px < 2^31, without forming the product (px can be close to 2^62)
bool below_2gib(long px, int bytes_per_px) { return px <= ((1L << 31) - 1) / bytes_per_px; }

int disp_elem(int format) { return format == DSM_DISP_F32 ? 4 : format == DSM_DISP_U8 ? 1 : 2; }

// Everything that is refused, in the order ARG, UNSUPPORTED, ALIGN.  Launches nothing.
int frames_check(const void* raw, size_t raw_bytes, const dsm_frame_source* srcs, const void* y,
                 const dsm_spatial_record* recs, int n_recs, int B, int C, int H0, int W0, int h, int w,
                 int to_tensor_channels) {
  DSM_REQUIRE(raw && srcs && y && recs, DSM_ERR_ARG);
  DSM_REQUIRE(B > 0 && H0 > 0 && W0 > 0 && h > 0 && w > 0, DSM_ERR_ARG);
  DSM_REQUIRE(C >= 6 && C <= 8, DSM_ERR_ARG);
  DSM_REQUIRE(n_recs == B, DSM_ERR_ARG);
  DSM_REQUIRE(to_tensor_channels == 0 || to_tensor_channels == 6, DSM_ERR_ARG);
  for (int i = 0; i < B; ++i) {
    DSM_REQUIRE(spatial_record_ok(recs[i], H0, W0, h, w), DSM_ERR_ARG);
    const dsm_frame_source& s = srcs[i];
    DSM_REQUIRE(s.Hs > 0 && s.Ws > 0 && s.y0 >= 0 && s.x0 >= 0, DSM_ERR_ARG);
    DSM_REQUIRE((long)s.y0 + H0 <= (long)s.Hs && (long)s.x0 + W0 <= (long)s.Ws, DSM_ERR_ARG);
    DSM_REQUIRE(s.flip == 0 || s.flip == 1, DSM_ERR_ARG);
    DSM_REQUIRE(s.disp_format >= DSM_DISP_F32 && s.disp_format <= DSM_DISP_U8, DSM_ERR_ARG);
    DSM_REQUIRE(plane_inside(s.imL, s.Hs, s.Ws, 3, raw_bytes), DSM_ERR_ARG);
    DSM_REQUIRE(plane_inside(s.imR, s.Hs, s.Ws, 3, raw_bytes), DSM_ERR_ARG);
    if (C >= 7) DSM_REQUIRE(plane_inside(s.dispL, s.Hs, s.Ws, disp_elem(s.disp_format), raw_bytes), DSM_ERR_ARG);
    if (C >= 8) DSM_REQUIRE(plane_inside(s.dispR, s.Hs, s.Ws, disp_elem(s.disp_format), raw_bytes), DSM_ERR_ARG);
  }
  // 32-bit element indices inside a plane, a frame and an output image
  DSM_REQUIRE(below_2gib((long)H0 * W0, 4 * C) && below_2gib((long)h * w, 4 * C), DSM_ERR_UNSUPPORTED);
  for (int i = 0; i < B; ++i) {
    const long px = (long)srcs[i].Hs * srcs[i].Ws;
    DSM_REQUIRE(below_2gib(px, 3), DSM_ERR_UNSUPPORTED);
    if (C >= 7) DSM_REQUIRE(below_2gib(px, disp_elem(srcs[i].disp_format)), DSM_ERR_UNSUPPORTED);
  }
  DSM_REQUIRE(((uintptr_t)y & 3u) == 0, DSM_ERR_ALIGN);
  for (int i = 0; i < B && C >= 7; ++i) {
    const uintptr_t mask = (uintptr_t)disp_elem(srcs[i].disp_format) - 1;     // 3, 1 or 0
    DSM_REQUIRE((((uintptr_t)raw + (uintptr_t)srcs[i].dispL) & mask) == 0, DSM_ERR_ALIGN);
    if (C >= 8) DSM_REQUIRE((((uintptr_t)raw + (uintptr_t)srcs[i].dispR) & mask) == 0, DSM_ERR_ALIGN);
  }
  return DSM_OK;
}

}  // namespace

extern "C" int dsm_stereo_spatial_raw_plan(const void* raw, size_t raw_bytes, const dsm_frame_source* srcs,
                                           void* y, const dsm_spatial_record* recs, int n_recs, int B,
                                           int C, int H0, int W0, int h, int w, int to_tensor_channels) {
  return frames_check(raw, raw_bytes, srcs, y, recs, n_recs, B, C, H0, W0, h, w, to_tensor_channels);
}

extern "C" int dsm_stereo_spatial_raw(const void* raw, size_t raw_bytes, const dsm_frame_source* srcs, void* y,
                                      const dsm_spatial_record* recs, int n_recs, int B, int C, int H0, int W0,
                                      int h, int w, int to_tensor_channels, dsm_stream_t stream) {
  const int ok = frames_check(raw, raw_bytes, srcs, y, recs, n_recs, B, C, H0, W0, h, w, to_tensor_channels);
  if (ok != DSM_OK) return ok;
  const long per_image = (long)h * w;
  long chunk = DSM_FRAMES_MAX_RECORDS;
  if (chunk * per_image >= (1L << 31)) chunk = ((1L << 31) - 1) / per_image;   // 32-bit work-item index
  dsm_clear_stale_error();
  for (int b0 = 0; b0 < B; b0 += (int)chunk) {
    const int nb = (int)(B - b0 < chunk ? B - b0 : chunk);
    FrameArgs a;
    ::memset(&a, 0, sizeof(a));
    ::memcpy(a.r, recs + b0, sizeof(dsm_spatial_record) * (size_t)nb);
    ::memcpy(a.s, srcs + b0, sizeof(dsm_frame_source) * (size_t)nb);
    const int blocks = dsm_cdiv((long)nb * per_image, 256);
    const int grid = blocks < 4096 ? blocks : 4096;
    auto kernel = C == 6 ? stereo_spatial_raw_kernel<6> : C == 7 ? stereo_spatial_raw_kernel<7>
                                                                 : stereo_spatial_raw_kernel<8>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)raw, (float*)y, a, b0, nb, W0, h, w, to_tensor_channels);
    const int st = dsm_launch_status();
    if (st != DSM_OK) return st;
  }
  return DSM_OK;
}
