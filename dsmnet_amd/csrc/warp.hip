// Disparity warp fused with the reconstruction error:
//   utils/imwrap.py:37-72  imwrap_BCHW(im_src, disp)  (defaults: fliplr False, LeftTop [0,0], scale 1)
//   models/iresnet.py:169-170  reconerror = |deconv1L2L - imwrap_BCHW(deconv1R2R, -r_pr0)|
// Stock torch spends ~8 launches and 5 passes over the (B,32,H,W) maps on this (linspace grids,
// stack, `im_src + delt`, grid_sample, sub, abs); here one pass: every map is read once and the
// error written once (3 x 63 MB at 384x1280 -> HBM-bound).
// Training (option `warp_train`): the same forward launch, and warp_abs_error_bwd_kernel below.
//
// Arithmetic follows this container's torch exactly where it matters: torch.linspace's
// two-sided fp32 formula for the base grid, grid_sample(bilinear, zeros, align_corners=False)
// un-normalisation ((g + 1) * size - 1) / 2 and its tap order nw, ne, sw, se; the reference's
// `+ delt` is applied to in-bounds taps only (out-of-bounds taps of `im_src + delt` are zeros).
#include "common.hpp"

namespace {

__global__ __launch_bounds__(256) void warp_abs_error_kernel(
    const float* __restrict__ L, const float* __restrict__ R, const float* __restrict__ disp,
    float* __restrict__ out, int C, int H, int W, int H0, int W0, float x1, float y1, float delt,
    int ncg) {
  // thread = (pixel, group of 8 channels): the r01 form walked all C channels per pixel, one
  // dependent iteration after the other (80 us for 189 MB); here the eight channels' taps are all
  // in flight together and the grid is ncg times as large
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y, b = blockIdx.z / ncg, c0 = (blockIdx.z % ncg) * 8;
  if (x >= W) return;
  const float d = disp[((long)b * H + y) * W + x];
  const dsm_warp_taps T = dsm_warp_taps_at(d, x, y, H, W, H0, W0, x1, y1);
  const long plane0 = (long)H0 * W0, plane = (long)H * W;
  const float* r = R + ((long)b * C + c0) * plane0 + (long)T.y0 * W0 + T.x0;
  const long o = ((long)b * C + c0) * plane + (long)y * W + x;
  const int nc = min(8, C - c0);
  float t[8][4], lv[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {                  // every load of the group issued before the first use
    const float* rc = r + (c < nc ? c : 0) * plane0;
    t[c][0] = T.i00 ? rc[0] : 0.f;
    t[c][1] = T.i01 ? rc[1] : 0.f;
    t[c][2] = T.i10 ? rc[W0] : 0.f;
    t[c][3] = T.i11 ? rc[W0 + 1] : 0.f;
    lv[c] = L ? L[o + (c < nc ? c : 0) * plane] : 0.f;
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    if (c >= nc) break;
    const float v = dsm_warp_sample(T, t[c][0], t[c][1], t[c][2], t[c][3], delt);   // the r01 form's sum order
    out[o + c * plane] = L ? fabsf(lv[c] - v) : v;
  }
}

// Backward of the kernel above (training: models/iresnet.py:169-170 under autograd).  Nothing is saved
// by the forward: grid, floor, clamp, in-bounds flags and the sum order of v are recomputed with the very
// same expressions, so sign(L - v) is taken of the value the forward produced.
//   gL    = g * sign(L - v)                                    one writer per element
//   gR   += gv * w_tap on every in-bounds tap, gv = -g * sign  fp32 global atomics (zeroed by the entry point)
//   gdisp = -(W0 / (W0 - 1)) * sum_c gv_c * (wy0 * (ne_c - nw_c) + wy1 * (se_c - sw_c))
//           with the tap values R + delt (0 out of bounds): ATen's grid_sample backward, zeros padding,
//           align_corners = False; dix/dgx * dgx/dd = (W0 / 2) * (-2 / (W0 - 1)); iy does not depend on disp
// Block = 64 consecutive pixels of one row x 4 channel groups of 8: every global access of a wave is one
// contiguous 256-byte row segment (the atomics too where the disparity is smooth), a thread has its eight
// channels' g, L and taps in flight together as in the forward, and the channel sum of gdisp is finished
// in a fixed order (registers, then four LDS slots), so gL and gdisp are run-to-run identical.
__global__ __launch_bounds__(256) void warp_abs_error_bwd_kernel(
    const float* __restrict__ G, const float* __restrict__ L, const float* __restrict__ R,
    const float* __restrict__ disp, float* __restrict__ gL, float* __restrict__ gR,
    float* __restrict__ gdisp, int C, int H, int W, int H0, int W0, float x1, float y1, float delt, int ncg) {
  __shared__ float part[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int x = blockIdx.x * 64 + tx, y = blockIdx.y, b = blockIdx.z;
  const bool valid = x < W;
  const int xc = valid ? x : W - 1;
  const float d = disp[((long)b * H + y) * W + xc];
  const dsm_warp_taps T = dsm_warp_taps_at(d, xc, y, H, W, H0, W0, x1, y1);
  const int x0 = T.x0, y0 = T.y0;
  const float wy0 = T.wy0, wy1 = T.wy1, nw = T.nw, ne = T.ne, sw = T.sw, se = T.se;
  const bool i00 = valid && T.i00, i01 = valid && T.i01, i10 = valid && T.i10, i11 = valid && T.i11;
  const long plane0 = (long)H0 * W0, plane = (long)H * W;
  float gsum = 0.f;
  for (int cg = ty; cg < ncg; cg += 4) {
    const int c0 = cg * 8, nc = min(8, C - c0);
    const long ro = ((long)b * C + c0) * plane0 + (long)y0 * W0 + x0;   // dereferenced behind i00..i11 only
    const long o = ((long)b * C + c0) * plane + (long)y * W + xc;
    float t[8][4], lv[8], gv[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {                // every load of the group issued before the first use
      const long rc = ro + (c < nc ? c : 0) * plane0, oc = o + (c < nc ? c : 0) * plane;
      t[c][0] = i00 ? R[rc] : 0.f;
      t[c][1] = i01 ? R[rc + 1] : 0.f;
      t[c][2] = i10 ? R[rc + W0] : 0.f;
      t[c][3] = i11 ? R[rc + W0 + 1] : 0.f;
      lv[c] = L ? L[oc] : 0.f;
      gv[c] = G[oc];
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (c >= nc || !valid) break;
      const float a = i00 ? t[c][0] + delt : 0.f, e = i01 ? t[c][1] + delt : 0.f;
      const float s = i10 ? t[c][2] + delt : 0.f, q = i11 ? t[c][3] + delt : 0.f;
      float v = 0.f;                             // the forward's sum, term for term
      if (i00) v += a * nw;
      if (i01) v += e * ne;
      if (i10) v += s * sw;
      if (i11) v += q * se;
      float gw = gv[c];                          // d loss / d v
      if (L) {
        const float df = lv[c] - v;
        const float sg = (float)(df > 0.f) - (float)(df < 0.f);      // torch.abs: 0 at equality
        const float gl = gv[c] * sg;
        if (gL) gL[o + c * plane] = gl;
        gw = -gl;
      }
      if (gR && gw != 0.f) {
        float* r = gR + ro + c * plane0;
        if (i00) unsafeAtomicAdd(r, gw * nw);
        if (i01) unsafeAtomicAdd(r + 1, gw * ne);
        if (i10) unsafeAtomicAdd(r + W0, gw * sw);
        if (i11) unsafeAtomicAdd(r + W0 + 1, gw * se);
      }
      gsum += gw * (wy0 * (e - a) + wy1 * (q - s));
    }
  }
  if (!gdisp) return;                            // uniform over the grid
  part[ty][tx] = gsum;
  __syncthreads();
  if (ty == 0 && valid)
    gdisp[((long)b * H + y) * W + x] =
        -((float)W0 / (float)(W0 - 1)) * (((part[0][tx] + part[1][tx]) + part[2][tx]) + part[3][tx]);
}

// a kernel, not hipMemsetAsync: a memset node does not replay reliably in a captured graph here
// (conv3d_bwd.hip, wgrad_zero_kernel)
__global__ __launch_bounds__(256) void warp_zero_kernel(float* __restrict__ p, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) p[i] = 0.f;
}

}  // namespace

extern "C" int dsm_warp_abs_error_bwd(const void* g, const void* L, const void* R, const void* disp,
                                      void* gL, void* gR, void* gdisp, int B, int C, int H, int W,
                                      int H0, int W0, float delt, dsm_stream_t stream) {
  DSM_REQUIRE(g && R && disp, DSM_ERR_ARG);
  DSM_REQUIRE(L || !gL, DSM_ERR_ARG);                                 // the plain warp has no left map
  DSM_REQUIRE(B > 0 && C > 0 && H <= 65535 && B <= 65535, DSM_ERR_ARG);
  DSM_REQUIRE(H > 1 && W > 1 && H0 > 1 && W0 > 1, DSM_ERR_ARG);      // imwrap.py:48
  const float x1 = (float)(-1.0 + (W - 1) * 2.0 / (W0 - 1));
  const float y1 = (float)(-1.0 + (H - 1) * 2.0 / (H0 - 1));
  dsm_clear_stale_error();
  if (gR) {
    const long n = (long)B * C * H0 * W0, blocks = (n + 255) / 256;
    hipLaunchKernelGGL(warp_zero_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0,
                       (hipStream_t)stream, (float*)gR, n);
  }
  if (gL || gR || gdisp)
    hipLaunchKernelGGL(warp_abs_error_bwd_kernel, dim3(dsm_cdiv(W, 64), H, B), dim3(256), 0,
                       (hipStream_t)stream, (const float*)g, (const float*)L, (const float*)R,
                       (const float*)disp, (float*)gL, (float*)gR, (float*)gdisp, C, H, W, H0, W0, x1, y1,
                       delt, (C + 7) / 8);
  return dsm_launch_status();
}

extern "C" int dsm_warp_abs_error(const void* L, const void* R, const void* disp, void* out, int B,
                                  int C, int H, int W, int H0, int W0, float delt,
                                  dsm_stream_t stream) {
  DSM_REQUIRE(R && disp && out, DSM_ERR_ARG);
  DSM_REQUIRE(B > 0 && C > 0 && H <= 65535, DSM_ERR_ARG);
  const int ncg = (C + 7) / 8;
  DSM_REQUIRE((long)B * ncg <= 65535, DSM_ERR_UNSUPPORTED);
  DSM_REQUIRE(H > 1 && W > 1 && H0 > 1 && W0 > 1, DSM_ERR_ARG);      // imwrap.py:48
  const float x1 = (float)(-1.0 + (W - 1) * 2.0 / (W0 - 1));
  const float y1 = (float)(-1.0 + (H - 1) * 2.0 / (H0 - 1));
  dsm_clear_stale_error();
  hipLaunchKernelGGL(warp_abs_error_kernel, dim3(dsm_cdiv(W, 256), H, B * ncg), dim3(256), 0,
                     (hipStream_t)stream, (const float*)L, (const float*)R, (const float*)disp,
                     (float*)out, C, H, W, H0, W0, x1, y1, delt, ncg);
  return dsm_launch_status();
}
