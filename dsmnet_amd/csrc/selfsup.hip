// Self-supervised "depthmono[-mask]" pyramid loss (losses/loss.py:196-236 loss_depthmono,
// :71-83 C_ds1, :393-405 weight_common, :424-467 losses_pyramid1; losses/SSIM.py:6-14, 24-42,
// 94-117; utils/imwrap.py:37-72 imwrap_BCHW with LeftTop / scale_factor / fliplr), fused.
//
// Stock torch spends ~220 small launches per (level, view) on this, forward and backward (3125
// for the preset pyramid, profiles/selfsup.md).  Here
// the whole pyramid (every level, both views) is ONE work list of 16x16 output tiles:
//   forward   selfsup_fwd_tiles   per tile: the image warp over the tile + 5-pixel halo, the five
//                                 channel-mean statistics, the separable 11-tap Gaussian in LDS,
//                                 SSIM, C_ap, C_ds1, the fliplr disparity warp, C_lr, the -mask
//                                 weights; per-tile partial sums to a slab, and 5 floats per pixel
//                                 saved for the backward (the SSIM partials and both candidate
//                                 weight_im maps: which one applies is known only after the
//                                 reduction, when the "< 1024 valid pixels" fallback is decided)
//             selfsup_reduce      one workgroup: the slabs summed in a fixed order (fp64), the
//                                 per-item means, simlary, w = wfun(simlary) and the weighted
//                                 pyramid total -- all on the device, no host read
//   backward  selfsup_bwd_tiles   per tile: the three saved SSIM partials (weighted) filtered
//                                 again by the same symmetric window (zero padding) = the SSIM
//                                 adjoint, the L1 sign, the bilinear derivative with respect to
//                                 the sample position (+delt on in-bounds taps included), C_ds1,
//                                 and the two cross-coupled left-right terms: disp is the sampling
//                                 offset of its own disp_wrap AND the sampled source of the other
//                                 view's, so the latter is a scatter (fp32 global atomics).
//
// Arithmetic follows this container's torch where it matters (see warp.hip): torch.linspace's
// two-sided fp32 formula, grid_sample(bilinear, zeros, align_corners=False) un-normalisation and
// tap order nw, ne, sw, se, `+ delt` on in-bounds taps only.  The masks follow the PyTorch 0.3
// meaning: mask2 = (delta < 3) & !(delta < 1), mask_im = (disp_wrap == 0)
// & mask_ap.  w, the masks and weight_common take no gradient, as in the reference.
//
// The "Cap[_ds][_lr][-mask]" objective (loss.py:238-283 loss_Cap_ds_lr) runs on the same kernels:
// the objective (Cap or depthmono), -mask and the two optional terms are template parameters of
// the tile kernels, chosen by the flags word (DSM_SELFSUP_*).  Cap differs in three ways: mask_ap
// has no "< 1024 valid pixels" fallback (so weight_im has one outcome and one saved plane; no
// valid pixel at all gives w = 0.001, Python's max(0, nan)), the smoothness weight is
// w / ds_divisor (per item), and C_ds / C_lr are there only when asked for.  Without the lr term
// nothing flows through disp_wrap: every gradient element has one writer, the backward is a pure
// gather that STORES every element (no atomics, no zeroed buffer, bit-reproducible), and without
// -mask the fliplr disparity warp is not computed at all.
//
// "common[-mask]" (loss.py:154-194 loss_common) is depthmono's rule with the depth-ratio smoothness
// C_ds3 (loss.py:99-114) in place of C_ds1: the instantiation <.., DS3 = true> of the tile kernels
// behind dsm_selfsup_ext_*, after a pre-pass (common_gradmean) that sums each batch sample's image
// gradients in a fixed order -- C_ds3's weights divide by their mean.
//
// "SsSMnet[-mask]" (loss.py:285-324 loss_SsSMnet through :469-512 losses_pyramid2) has kernels of its
// own behind the same entry points (sss_*, further down): a warp of a warp, an image-gradient term,
// second-order smoothness and a two-stage backward.
//
// What changes from step to step -- the epsilons of the warps and the level weights -- reaches the
// kernels either inside the by-value structs (read when the host launches) or, behind
// dsm_selfsup_dyn_*, from a device array that they read when they run (Work::params, step_scalars):
// the same kernels, so that a captured graph replays with every step's own numbers.
#include "common.hpp"

namespace {

constexpr int T = 16;                 // output tile edge
constexpr int HALO = 5;               // 11-tap window
constexpr int RW = T + 2 * HALO;      // 26: region edge
constexpr int NPART = 8;              // partial sums per tile (7 used)
constexpr int NSAVE = 5;              // floats saved per pixel
constexpr float C1 = 1e-4f, C2 = 9e-4f;   // (0.01)^2, (0.03)^2: SSIM.py:36-38
static_assert(sizeof(dsm_selfsup_item) == 128, "dsm_selfsup_item layout (ctypes mirror in _lib.py)");

struct Work {
  dsm_selfsup_item it[DSM_SELFSUP_MAX_ITEMS];
  int tile0[DSM_SELFSUP_MAX_ITEMS + 1];     // first tile of each item; tile0[n] = total
  int ntx[DSM_SELFSUP_MAX_ITEMS], nty[DSM_SELFSUP_MAX_ITEMS];
  long save0[DSM_SELFSUP_MAX_ITEMS];        // float offset of each item's saved planes
  float xs[DSM_SELFSUP_MAX_ITEMS], xe[DSM_SELFSUP_MAX_ITEMS];   // linspace ends (imwrap.py:53-56)
  float ys[DSM_SELFSUP_MAX_ITEMS], ye[DSM_SELFSUP_MAX_ITEMS];
  float g[11];                              // 1-D Gaussian, SSIM.py:6-8 (fp32, normalised)
  int n, flag_mask;
  float* part;                              // tile partial sums [tiles][NPART]
  float* save;                              // [item][NSAVE][B*h*w]
  // the objective, for the reduction (the tile kernels take it as template parameters); after the
  // older fields, whose offsets the depthmono instantiation keeps
  int cap, ds, lr;
  // common (C_ds3): partial sums of |diff1_dx(im)|, |diff1_dy(im)| as [item][gm_B][NCH][2]
  float* gmean;
  int gm_B;
  // the per-step scalars as a device array [n][4] = {delt_im, delt_disp, delt_im1, weight} per item,
  // read when the kernels run (dsm_selfsup_dyn_*: a captured graph replays with new values); NULL:
  // the items' own fields and Warps::delt1, read at launch.  Last, so that the older offsets stay
  const float* params;
};

// the per-step scalars of item i.  i comes from blockIdx: uniform per workgroup, one 16-byte load
// hoisted out of the pixel loops (check_params: the array is 16-byte aligned)
struct Step {
  float delt_im, delt_disp, delt_im1, weight;
};

__device__ __forceinline__ Step step_scalars(const Work& W, int i, float delt_im1 = 0.f) {
  if (W.params) {
    const float4 v = *(const float4*)(W.params + 4 * i);
    return Step{v.x, v.y, v.z, v.w};
  }
  return Step{W.it[i].delt_im, W.it[i].delt_disp, delt_im1, W.it[i].weight};
}

__device__ __forceinline__ float item_weight(const Work& W, int i) {
  return W.params ? W.params[4 * i + 3] : W.it[i].weight;
}

__device__ __forceinline__ float sgnf(float v) { return (float)((v > 0.f) - (v < 0.f)); }

// grid_sample's bilinear tap set at normalised (gx, gy) of a W0 x H0 plane
struct Bil {
  int x0, y0;
  float wx0, wx1, wy0, wy1;
  bool in00, in01, in10, in11;
};

__device__ __forceinline__ Bil bil_setup(float gx, float gy, int W0, int H0) {
  Bil t;
  const float ix = ((gx + 1.f) * (float)W0 - 1.f) / 2.f;
  const float iy = ((gy + 1.f) * (float)H0 - 1.f) / 2.f;
  const float fx = floorf(ix), fy = floorf(iy);
  // wild disparities: clamp before the int conversion (the taps then fall outside, as in torch)
  t.x0 = (int)fminf(fmaxf(fx, -2.f), (float)W0 + 1.f);
  t.y0 = (int)fminf(fmaxf(fy, -2.f), (float)H0 + 1.f);
  t.wx1 = ix - fx; t.wx0 = (fx + 1.f) - ix;
  t.wy1 = iy - fy; t.wy0 = (fy + 1.f) - iy;
  const bool x0in = t.x0 >= 0 && t.x0 < W0, x1in = t.x0 + 1 >= 0 && t.x0 + 1 < W0;
  const bool y0in = t.y0 >= 0 && t.y0 < H0, y1in = t.y0 + 1 >= 0 && t.y0 + 1 < H0;
  t.in00 = y0in && x0in; t.in01 = y0in && x1in; t.in10 = y1in && x0in; t.in11 = y1in && x1in;
  return t;
}

// value of (plane + delt) at the taps (zeros outside) and its derivative with respect to ix
__device__ __forceinline__ void bil_sample(const float* p, int sy, int sx, const Bil& t, float delt,
                                           float& v, float& dvx) {
  const float a = t.in00 ? p[(long)t.y0 * sy + (long)t.x0 * sx] + delt : 0.f;
  const float b = t.in01 ? p[(long)t.y0 * sy + (long)(t.x0 + 1) * sx] + delt : 0.f;
  const float c = t.in10 ? p[(long)(t.y0 + 1) * sy + (long)t.x0 * sx] + delt : 0.f;
  const float d = t.in11 ? p[(long)(t.y0 + 1) * sy + (long)(t.x0 + 1) * sx] + delt : 0.f;
  float s = 0.f;                                   // torch's order: nw, ne, sw, se
  if (t.in00) s += a * (t.wx0 * t.wy0);
  if (t.in01) s += b * (t.wx1 * t.wy0);
  if (t.in10) s += c * (t.wx0 * t.wy1);
  if (t.in11) s += d * (t.wx1 * t.wy1);
  v = s;
  dvx = (b - a) * t.wy0 + (d - c) * t.wy1;
}

struct Pix {            // one output pixel of one item
  const dsm_selfsup_item* it;
  int i, b, y, x;
  float delt_im, delt_disp;   // of step_scalars
};

// image warp at (y, x): im_wrap channels and their d/dix; the raw image channels too
__device__ __forceinline__ void image_warp(const Work& W, const Pix& q, float d, float iw[3],
                                           float div[3], float im[3]) {
  const dsm_selfsup_item& it = *q.it;
  const float gx = linspace_at(W.xs[q.i], W.xe[q.i], it.w, q.x) - d * 2.0f / (float)(it.W0 - 1);
  const float gy = linspace_at(W.ys[q.i], W.ye[q.i], it.h, q.y);
  const Bil t = bil_setup(gx, gy, it.W0, it.H0);
  const float* src = (const float*)it.src + (long)q.b * it.src_stride[0];
  const float* imp = (const float*)it.im + (long)q.b * it.im_stride[0] + (long)q.y * it.im_stride[2] +
                     (long)q.x * it.im_stride[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    bil_sample(src + (long)c * it.src_stride[1], it.src_stride[2], it.src_stride[3], t, q.delt_im,
               iw[c], div[c]);
    im[c] = imp[(long)c * it.im_stride[1]];
  }
}

// fliplr disparity warp (imwrap.py:57-70 with fliplr=True, LeftTop [0,0], scale 1): disp_other
// sampled at -(linspace(-1, 1) - d * 2 / (w - 1)); returns the tap set for the scatter
__device__ __forceinline__ Bil disp_warp(const Pix& q, float d, float& dw, float& ddw) {
  const dsm_selfsup_item& it = *q.it;
  const float gx = -(linspace_at(-1.f, 1.f, it.w, q.x) - d * 2.0f / (float)(it.w - 1));
  const float gy = linspace_at(-1.f, 1.f, it.h, q.y);
  const Bil t = bil_setup(gx, gy, it.w, it.h);
  bil_sample((const float*)it.disp_other + (long)q.b * it.h * it.w, it.w, 1, t, q.delt_disp, dw, ddw);
  return t;
}

__device__ __forceinline__ float weight_common(float d, float dw, int factor) {   // loss.py:393-405
  const float delta = fabsf(d - dw) / (float)factor;
  return delta < 1.f ? 1.f : (delta < 3.f ? 1.f - (delta - 1.f) * (0.99f / 2.f) : 0.01f);
}

__device__ __forceinline__ int find_item(const Work& W, int tile) {
  int i = 0;
  while (i + 1 < W.n && tile >= W.tile0[i + 1]) ++i;
  return i;
}

__device__ __forceinline__ void tile_origin(const Work& W, int i, int tile, int& b, int& ty0, int& tx0) {
  int local = tile - W.tile0[i];
  const int per = W.ntx[i] * W.nty[i];
  b = local / per;
  local -= b * per;
  ty0 = (local / W.ntx[i]) * T;
  tx0 = (local % W.ntx[i]) * T;
}

// separable 11-tap filter of NS LDS maps: region [NS][RW][RW+1] -> value at (ty, tx) of the tile
template <int NS>
__device__ __forceinline__ void filter_tile(const Work& W, float (*reg)[RW][RW + 1],
                                            float (*hs)[RW][T + 1], float out[NS]) {
  for (int r = threadIdx.x; r < RW * T; r += blockDim.x) {
    const int row = r / T, col = r % T;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 11; ++j) s += W.g[j] * reg[k][row][col + j];
      hs[k][row][col] = s;
    }
  }
  __syncthreads();
  const int ty = threadIdx.x / T, tx = threadIdx.x % T;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 11; ++j) s += W.g[j] * hs[k][ty + j][tx];
    out[k] = s;
  }
}

// ---- common's smoothness C_ds3 (loss.py:99-114, diff_z_dx/dy :56-64) --------------------------
constexpr int NCH = 16;               // row chunks per (item, sample) of the image-gradient pre-pass

// sum |diff1_dx(im)| and sum |diff1_dy(im)| of one row chunk of one (item, sample): every sum in a
// fixed order (fp64 per thread, LDS tree), so that the weights and with them the loss are
// bit-reproducible
__global__ __launch_bounds__(256) void common_gradmean(const Work W) {
  __shared__ double red[2][256];
  const int i = blockIdx.z, b = blockIdx.y, ch = blockIdx.x;
  const dsm_selfsup_item& it = W.it[i];
  if (b >= it.B) return;
  const int h = it.h, w = it.w;
  const int r0 = (int)((long)h * ch / NCH), rows = (int)((long)h * (ch + 1) / NCH) - r0;
  const float* im = (const float*)it.im + (long)b * it.im_stride[0];
  double sx = 0.0, sy = 0.0;
  for (int e = threadIdx.x; e < 3 * rows * w; e += blockDim.x) {      // make_work: 3 h w < 2^31
    const int x = e % w, t = e / w;
    const int y = r0 + t % rows, c = t / rows;
    const float* p = im + (long)c * it.im_stride[1] + (long)y * it.im_stride[2] + (long)x * it.im_stride[3];
    const float v = p[0];
    if (x + 1 < w) sx += (double)fabsf(p[it.im_stride[3]] - v);
    if (y + 1 < h) sy += (double)fabsf(p[it.im_stride[2]] - v);
  }
  red[0][threadIdx.x] = sx;
  red[1][threadIdx.x] = sy;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      red[0][threadIdx.x] += red[0][threadIdx.x + o];
      red[1][threadIdx.x] += red[1][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x < 2) W.gmean[((long)(i * W.gm_B + b) * NCH + ch) * 2 + threadIdx.x] = (float)red[threadIdx.x][0];
}

// 0.5 * mean over (C, H, W) of |diff1_dx(im)| and of |diff1_dy(im)| of sample b of item i
__device__ __forceinline__ void half_gradmean(const Work& W, int i, int b, float& hx, float& hy) {
  const float* gm = W.gmean + (long)(i * W.gm_B + b) * NCH * 2;
  double sx = 0.0, sy = 0.0;
  for (int c = 0; c < NCH; ++c) {
    sx += (double)gm[2 * c];
    sy += (double)gm[2 * c + 1];
  }
  const double n = 3.0 * (double)W.it[i].h * (double)W.it[i].w;
  hx = 0.5f * (float)(sx / n);
  hy = 0.5f * (float)(sy / n);
}

__device__ __forceinline__ float dz(float d) { return fabsf(d) + 1.f; }
// diff_z at centre c between m and p (all |disp| + 1), before abs and clamp
__device__ __forceinline__ float ratio2(float m, float c, float p) { return c / p + c / m - 2.f; }
// d clamp(|r|, 0, 10) / d r, as torch differentiates it (the bound passes)
__device__ __forceinline__ float clamp_sgn(float r) { return fabsf(r) <= 10.f ? sgnf(r) : 0.f; }
// exp(-max_c |im[+step] - im| / (0.5 m)) at a pixel whose forward neighbour exists
__device__ __forceinline__ float ds3_weight(const float* imp, int cs, int step, float half_m) {
  float e = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) e = fmaxf(e, fabsf(imp[(long)c * cs + step] - imp[(long)c * cs]));
  return expf(-(e / half_m));
}

// one axis of C_ds3 at position pos of len: dp / imp point at the pixel, s / step are the strides
__device__ __forceinline__ float ds3_fwd(const float* dp, int s, int pos, int len, const float* imp, int cs,
                                         int step, float half_m) {
  if (pos < 1 || pos + 1 >= len) return 0.f;
  const float r = ratio2(dz(dp[-s]), dz(dp[0]), dz(dp[s]));
  return fminf(fabsf(r), 10.f) * ds3_weight(imp, cs, step, half_m);
}

// its derivative with respect to the pixel's disparity: the pixel is the centre of its own term
// and the neighbour in the terms of pos - 1 and pos + 1
__device__ __forceinline__ float ds3_bwd(const float* dp, int s, int pos, int len, const float* imp, int cs,
                                         int step, float half_m) {
  const float a = dz(dp[0]);
  float g = 0.f;
  if (pos >= 1 && pos + 1 < len) {
    const float m = dz(dp[-s]), p = dz(dp[s]);
    g += clamp_sgn(ratio2(m, a, p)) * ds3_weight(imp, cs, step, half_m) * (1.f / p + 1.f / m);
  }
  if (pos >= 2) {
    const float c = dz(dp[-s]);
    g -= clamp_sgn(ratio2(dz(dp[-2 * s]), c, a)) * ds3_weight(imp - step, cs, step, half_m) * (c / (a * a));
  }
  if (pos + 2 < len) {
    const float c = dz(dp[s]);
    g -= clamp_sgn(ratio2(a, c, dz(dp[2 * s]))) * ds3_weight(imp + step, cs, step, half_m) * (c / (a * a));
  }
  return g * sgnf(dp[0]);
}

// CAP: loss_Cap_ds_lr's rule (no fallback), else loss_depthmono's; MASK: the -mask weights;
// DS / LR: the smoothness and left-right terms.  depthmono is the ONE instantiation
// <false, false, true, true>: it has both terms and reads -mask from W.flag_mask at run time, as
// it always did, so that it compiles to the instructions it had before the Cap rule existed.
// DS3: common -- depthmono's rule and instantiation with C_ds3 in place of C_ds1
template <bool CAP, bool MASK>
__device__ __forceinline__ bool has_mask(const Work& W) { return CAP ? MASK : W.flag_mask != 0; }

template <bool CAP, bool MASK, bool DS, bool LR, bool DS3 = false>
__global__ __launch_bounds__(256) void selfsup_fwd_tiles(const Work W) {
  __shared__ float reg[5][RW][RW + 1];
  __shared__ float hs[5][RW][T + 1];
  __shared__ float red[4][NPART];
  __shared__ float hm[2];               // DS3: 0.5 * the sample's mean image gradients, x and y
  const int tile = blockIdx.x;
  const int i = find_item(W, tile);
  const dsm_selfsup_item& it = W.it[i];
  int b, ty0, tx0;
  tile_origin(W, i, tile, b, ty0, tx0);
  const Step P = step_scalars(W, i);
  const int h = it.h, w = it.w;
  const float* disp = (const float*)it.disp + (long)b * h * w;
  if (DS3 && threadIdx.x == 0) half_gradmean(W, i, b, hm[0], hm[1]);   // once per tile; read after the barrier below

  // 1. statistics over the tile + halo (zero outside the map: conv2d's zero padding)
  for (int r = threadIdx.x; r < RW * RW; r += blockDim.x) {
    const int ry = r / RW, rx = r % RW;
    const int y = ty0 - HALO + ry, x = tx0 - HALO + rx;
    float m1 = 0.f, m2 = 0.f, q11 = 0.f, q22 = 0.f, q12 = 0.f;
    if (y >= 0 && y < h && x >= 0 && x < w) {
      const Pix q{&it, i, b, y, x, P.delt_im, P.delt_disp};
      float iw[3], div[3], im[3];
      image_warp(W, q, disp[(long)y * w + x], iw, div, im);
      m1 = (im[0] + im[1] + im[2]) / 3.f;
      m2 = (iw[0] + iw[1] + iw[2]) / 3.f;
      q11 = (im[0] * im[0] + im[1] * im[1] + im[2] * im[2]) / 3.f;
      q22 = (iw[0] * iw[0] + iw[1] * iw[1] + iw[2] * iw[2]) / 3.f;
      q12 = (im[0] * iw[0] + im[1] * iw[1] + im[2] * iw[2]) / 3.f;
    }
    reg[0][ry][rx] = m1; reg[1][ry][rx] = m2; reg[2][ry][rx] = q11; reg[3][ry][rx] = q22;
    reg[4][ry][rx] = q12;
  }
  __syncthreads();
  float st[5];
  filter_tile<5>(W, reg, hs, st);

  // 2. the pixel's terms
  const int y = ty0 + threadIdx.x / T, x = tx0 + threadIdx.x % T;
  float part[NPART] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (y < h && x < w) {
    const Pix q{&it, i, b, y, x, P.delt_im, P.delt_disp};
    const long o = (long)y * w + x;
    const float d = disp[o];
    float iw[3], div[3], im[3];
    image_warp(W, q, d, iw, div, im);
    const float mu1 = st[0], mu2 = st[1];
    const float A1 = 2.f * mu1 * mu2 + C1;
    const float A2 = 2.f * (st[4] - mu1 * mu2) + C2;
    const float B1 = mu1 * mu1 + mu2 * mu2 + C1;
    const float B2 = (st[2] - mu1 * mu1) + (st[3] - mu2 * mu2) + C2;
    const float inv = 1.f / (B1 * B2);
    const float S = A1 * A2 * inv;
    const float dS_mu2 = 2.f * mu1 * (A2 - A1) * inv - 2.f * mu2 * S * (1.f / B1 - 1.f / B2);
    const float dS_e22 = -S / B2;
    const float dS_e12 = 2.f * A1 * inv;
    float dw = 0.f, ddw;
    if (!CAP || MASK || LR) disp_warp(q, d, dw, ddw);         // Cap with neither: disp_other is never read
    // mask_ap and the weight switches test exact zeros (a sample with all four taps outside):
    // steps in the loss, so a sample within rounding of the border may fall either way in fp32
    // and fp64 -- the GPU tests bound the fraction of such pixels instead of their error
    const bool valid = iw[0] != 0.f;                          // mask_ap (loss.py:199)
    float wimA = 1.f, wimB = 1.f, wlr = 1.f;
    if (has_mask<CAP, MASK>(W)) {
      const float wc = weight_common(d, dw, it.scale_factor);
      wimA = (dw == 0.f && valid) ? 1.f : wc;                  // mask_im with the real mask_ap
      wimB = (dw == 0.f) ? 1.f : wc;                           // ... with the fallback mask_ap = 1
      wlr = (dw == 0.f) ? 0.f : wc;
    }
    const float ap = 3.f * 0.425f * (1.f - S) +
                     0.15f * (fabsf(im[0] - iw[0]) + fabsf(im[1] - iw[1]) + fabsf(im[2] - iw[2]));
    // C_ds1: forward differences, zero in the last column / row (diff1_dx / diff1_dy)
    const float* imp = (const float*)it.im + (long)b * it.im_stride[0] + (long)y * it.im_stride[2] +
                       (long)x * it.im_stride[3];
    float ds = 0.f;
    if (DS3) {
      ds = ds3_fwd(disp + o, 1, x, w, imp, it.im_stride[1], it.im_stride[3], hm[0]) +
           ds3_fwd(disp + o, w, y, h, imp, it.im_stride[1], it.im_stride[2], hm[1]);
    }
    if (!DS3 && DS && x + 1 < w) {
      float e = 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) e += fabsf(imp[(long)c * it.im_stride[1] + it.im_stride[3]] - im[c]);
      ds += fabsf(disp[o + 1] - d) * expf(-e);
    }
    if (!DS3 && DS && y + 1 < h) {
      float e = 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) e += fabsf(imp[(long)c * it.im_stride[1] + it.im_stride[2]] - im[c]);
      ds += fabsf(disp[o + w] - d) * expf(-e);
    }
    part[0] = wimA * ap;
    if (!CAP) part[1] = wimB * ap;
    part[2] = ds;
    if (LR) part[3] = wlr * fabsf(d - dw);
    part[4] = valid ? S : 0.f;
    part[5] = valid ? 1.f : 0.f;
    if (!CAP) part[6] = S;
    const long n = (long)it.B * h * w, p = (long)b * h * w + o;
    float* sv = W.save + W.save0[i];
    sv[p] = dS_mu2;
    sv[n + p] = dS_e22;
    sv[2 * n + p] = dS_e12;
    if (!CAP || MASK) sv[3 * n + p] = wimA;                   // Cap without -mask: weight_im = 1
    if (!CAP) sv[4 * n + p] = wimB;
  }
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll
  for (int k = 0; k < NPART; ++k) {
    const float s = wave_sum(part[k]);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < NPART) {
    const int k = threadIdx.x;
    W.part[(long)tile * NPART + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

// one workgroup; every sum in a fixed order (fp64), so the loss is bit-reproducible
__global__ __launch_bounds__(256) void selfsup_reduce(const Work W, float* loss, float* aux) {
  __shared__ double red[256];
  __shared__ double sums[DSM_SELFSUP_MAX_ITEMS][7];
  for (int i = 0; i < W.n; ++i) {
    for (int k = 0; k < 7; ++k) {
      double s = 0.0;
      for (int t = W.tile0[i] + threadIdx.x; t < W.tile0[i + 1]; t += blockDim.x)
        s += (double)W.part[(long)t * NPART + k];
      red[threadIdx.x] = s;
      __syncthreads();
      for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
      }
      if (threadIdx.x == 0) sums[i][k] = red[0];
      __syncthreads();
    }
  }
  if (threadIdx.x != 0) return;
  double total = 0.0;
  for (int i = 0; i < W.n; i += 2) {
    double C[2];
    for (int s = 0; s < 2; ++s) {
      const int j = i + s;
      const double n = (double)W.it[j].B * W.it[j].h * W.it[j].w;
      const double count = sums[j][5];
      if (W.cap) {
        // loss.py:241-243, 266-277: the mean over mask_ap however few pixels that is.  None at
        // all: the reference's empty mean is NaN and Python's max(0, nan) is 0, so w = 0.001;
        // count never divides into anything that reaches the loss
        const bool any = count > 0.0;
        const double simlary = any ? sums[j][4] / count : 0.0;
        const double wt = any ? fmax(0.0, simlary - 0.75) / 2.0 + 0.001 : 0.001;
        const int dv = W.it[j].ds_divisor > 0 ? W.it[j].ds_divisor : 1;
        double c = sums[j][0] / (3.0 * n);
        if (W.ds) c += (sums[j][2] / n) * (wt / (double)dv);
        if (W.lr) c += (sums[j][3] / n) * wt;
        C[s] = c;
        aux[4 * j + 0] = (float)wt;
        aux[4 * j + 1] = 0.f;
        aux[4 * j + 2] = (float)c;
        aux[4 * j + 3] = (float)simlary;
        continue;
      }
      const bool fallback = count < 1024.0;                   // loss.py:200-201
      const double simlary = fallback ? sums[j][6] / n : sums[j][4] / count;
      const double wt = fmax(0.0, simlary - 0.75) / 2.0 + 0.001;   // wfun, loss.py:33-34
      const double ap = (fallback ? sums[j][1] : sums[j][0]) / (3.0 * n);
      C[s] = ap + wt * (sums[j][2] / n) + wt * (sums[j][3] / n);
      aux[4 * j + 0] = (float)wt;
      aux[4 * j + 1] = fallback ? 1.f : 0.f;
      aux[4 * j + 2] = (float)C[s];
      aux[4 * j + 3] = (float)simlary;
    }
    total += (C[0] + C[1]) * (double)item_weight(W, i);
  }
  loss[0] = (float)total;
}

template <bool CAP, bool MASK, bool DS, bool LR, bool DS3 = false>
__global__ __launch_bounds__(256) void selfsup_bwd_tiles(const Work W, const float* __restrict__ aux,
                                                         const float* __restrict__ gloss) {
  __shared__ float reg[3][RW][RW + 1];
  __shared__ float hs[3][RW][T + 1];
  const int tile = blockIdx.x;
  const int i = find_item(W, tile);
  const dsm_selfsup_item& it = W.it[i];
  int b, ty0, tx0;
  tile_origin(W, i, tile, b, ty0, tx0);
  const Step P = step_scalars(W, i);
  const int h = it.h, w = it.w;
  const long n = (long)it.B * h * w;
  const float* sv = W.save + W.save0[i];
  const float wt = aux[4 * i + 0];
  const bool fallback = !CAP && aux[4 * i + 1] != 0.f;
  const float* wim_plane = sv + (fallback ? 4 : 3) * n;
  constexpr bool unit_wim = CAP && !MASK;                     // no plane was saved: weight_im = 1
  const float wds = CAP ? wt / (float)(it.ds_divisor > 0 ? it.ds_divisor : 1) : wt;   // loss.py:272
  const float gs = gloss[0] * P.weight;
  const float inv_n = 1.f / (float)n;
  const float* disp = (const float*)it.disp + (long)b * h * w;
  __shared__ float hm[2];               // DS3: as in the forward
  if (DS3 && threadIdx.x == 0) half_gradmean(W, i, b, hm[0], hm[1]);

  // 1. the weighted SSIM partials over tile + halo, zero outside the map
  for (int r = threadIdx.x; r < RW * RW; r += blockDim.x) {
    const int ry = r / RW, rx = r % RW;
    const int y = ty0 - HALO + ry, x = tx0 - HALO + rx;
    float p0 = 0.f, p1 = 0.f, p2 = 0.f;
    if (y >= 0 && y < h && x >= 0 && x < w) {
      const long p = (long)b * h * w + (long)y * w + x;
      const float wim = unit_wim ? 1.f : wim_plane[p];
      p0 = wim * sv[p]; p1 = wim * sv[n + p]; p2 = wim * sv[2 * n + p];
    }
    reg[0][ry][rx] = p0; reg[1][ry][rx] = p1; reg[2][ry][rx] = p2;
  }
  __syncthreads();
  float F[3];
  filter_tile<3>(W, reg, hs, F);

  const int y = ty0 + threadIdx.x / T, x = tx0 + threadIdx.x % T;
  if (y >= h || x >= w) return;
  const Pix q{&it, i, b, y, x, P.delt_im, P.delt_disp};
  const long o = (long)y * w + x, p = (long)b * h * w + o;
  const float d = disp[o];
  float iw[3], div[3], im[3];
  image_warp(W, q, d, iw, div, im);
  const float wim = unit_wim ? 1.f : wim_plane[p];

  // 2. C_ap: d C / d im_wrap_c, then through the sample position (imwrap.py:67: dix/dd = -W0/(W0-1))
  float gix = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float giw = (-0.425f / 3.f) * inv_n * (F[0] + 2.f * iw[c] * F[1] + im[c] * F[2]) +
                      (0.15f / 3.f) * inv_n * wim * sgnf(iw[c] - im[c]);
    gix += giw * div[c];
  }
  float gd = gix * (-(float)it.W0 / (float)(it.W0 - 1));

  // 3. C_lr = |d - d_wrap| * weight_lr: d is the offset of its own warp and the source of the
  //    other view's warp (scattered there: the other item's d_wrap taps land in this grad_other)
  //    Without the term nothing reaches disp_wrap (the weights are detached): no warp, no scatter
  if (LR) {
    float dw, ddw;
    const Bil t = disp_warp(q, d, dw, ddw);
    const float wlr = has_mask<CAP, MASK>(W) ? ((dw == 0.f) ? 0.f : weight_common(d, dw, it.scale_factor)) : 1.f;
    const float s = sgnf(d - dw) * wlr * wt * inv_n;
    gd += s;
    gd += -s * ddw * ((float)w / (float)(w - 1));
    if (s != 0.f) {
      float* go = (float*)it.grad_other + (long)b * h * w;
      const float v = -s * gs;
      if (t.in00) unsafeAtomicAdd(go + (long)t.y0 * w + t.x0, v * (t.wx0 * t.wy0));
      if (t.in01) unsafeAtomicAdd(go + (long)t.y0 * w + t.x0 + 1, v * (t.wx1 * t.wy0));
      if (t.in10) unsafeAtomicAdd(go + (long)(t.y0 + 1) * w + t.x0, v * (t.wx0 * t.wy1));
      if (t.in11) unsafeAtomicAdd(go + (long)(t.y0 + 1) * w + t.x0 + 1, v * (t.wx1 * t.wy1));
    }
  }

  // 4. C_ds1: the pixel is the right end of (x-1, x) and the left end of (x, x+1); same in y
  const float* imp = (const float*)it.im + (long)b * it.im_stride[0] + (long)y * it.im_stride[2] +
                     (long)x * it.im_stride[3];
  const int cs = it.im_stride[1], xs = it.im_stride[3], ys = it.im_stride[2];
  float gds = 0.f;
  if (DS3) gds = ds3_bwd(disp + o, 1, x, w, imp, cs, xs, hm[0]) + ds3_bwd(disp + o, w, y, h, imp, cs, ys, hm[1]);
  if (!DS3 && DS && x + 1 < w) {
    float e = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) e += fabsf(imp[(long)c * cs + xs] - im[c]);
    gds -= sgnf(disp[o + 1] - d) * expf(-e);
  }
  if (!DS3 && DS && x > 0) {
    float e = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) e += fabsf(im[c] - imp[(long)c * cs - xs]);
    gds += sgnf(d - disp[o - 1]) * expf(-e);
  }
  if (!DS3 && DS && y + 1 < h) {
    float e = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) e += fabsf(imp[(long)c * cs + ys] - im[c]);
    gds -= sgnf(disp[o + w] - d) * expf(-e);
  }
  if (!DS3 && DS && y > 0) {
    float e = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) e += fabsf(im[c] - imp[(long)c * cs - ys]);
    gds += sgnf(d - disp[o - w]) * expf(-e);
  }
  gd += gds * wds * inv_n;
  // with the lr term the other view's scatter lands here too (accumulate into the zeroed buffer);
  // without it this thread is the element's only writer: a plain store, whatever was there
  if (LR) unsafeAtomicAdd((float*)it.grad_disp + p, gd * gs);
  else ((float*)it.grad_disp)[p] = gd * gs;
}


// ---- SsSMnet[-mask] (loss.py:285-324 loss_SsSMnet, :469-512 losses_pyramid2, :85-97 C_ds2, :66-69
// C_imdiff1) ----------------------------------------------------------------------------------
// im_wrap1 of a view samples the OTHER view's warped image, which other workgroups produce: a first
// launch materialises every item's im_wrap (3 floats per pixel); the tile kernel then reads its own
// item's buffer over tile + halo and at the +1 neighbours (C_imdiff1) and the other item's at the
// four taps of the fliplr grid.  Backward, two stages: d C_lr / d im_wrap of the other view arrives
// as a scatter (fp32 atomics, <= 4 taps x 3 channels per pixel) into a zeroed buffer per item, and a
// second launch takes it through d im_wrap / d ix to the disparity; everything else is a gather by
// the pixel's own thread, which stores its element.
struct Warps {
  float* warp[DSM_SELFSUP_MAX_ITEMS];       // (B,3,h,w) im_wrap of each item
  float* gwarp[DSM_SELFSUP_MAX_ITEMS];      // (B,3,h,w) scattered d loss / d im_wrap (backward)
  float delt1[DSM_SELFSUP_MAX_ITEMS];       // the epsilon of im_wrap1
};

__global__ __launch_bounds__(256) void sss_warp(const Work W, const Warps E) {
  const int tile = blockIdx.x;
  const int i = find_item(W, tile);
  const dsm_selfsup_item& it = W.it[i];
  int b, ty0, tx0;
  tile_origin(W, i, tile, b, ty0, tx0);
  const Step P = step_scalars(W, i, E.delt1[i]);
  const int y = ty0 + threadIdx.x / T, x = tx0 + threadIdx.x % T;
  if (y >= it.h || x >= it.w) return;
  const Pix q{&it, i, b, y, x, P.delt_im, P.delt_disp};
  const long hw = (long)it.h * it.w, o = (long)y * it.w + x;
  float iw[3], div[3], im[3];
  image_warp(W, q, ((const float*)it.disp)[b * hw + o], iw, div, im);
#pragma unroll
  for (int c = 0; c < 3; ++c) E.warp[i][(b * 3L + c) * hw + o] = iw[c];
}

// the fliplr grid of imwrap(.., fliplr=True, LeftTop [0,0], scale 1) at (y, x): disp_warp's
__device__ __forceinline__ Bil flip_taps(const dsm_selfsup_item& it, int y, int x, float d) {
  const float gx = -(linspace_at(-1.f, 1.f, it.w, x) - d * 2.0f / (float)(it.w - 1));
  return bil_setup(gx, linspace_at(-1.f, 1.f, it.h, y), it.w, it.h);
}

// one axis of C_ds2 at position pos of len: |second difference of disp| * exp(-sum_c |second
// difference of im|), zero at both ends
__device__ __forceinline__ float ds2_weight(const float* imp, int cs, int step) {
  float e = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) e += fabsf(imp[(long)c * cs + step] + imp[(long)c * cs - step] - 2.f * imp[(long)c * cs]);
  return expf(-e);
}
__device__ __forceinline__ float diff2(const float* dp, int s) { return dp[s] + dp[-s] - dp[0] - dp[0]; }

__device__ __forceinline__ float ds2_bwd(const float* dp, int s, int pos, int len, const float* imp, int cs, int step) {
  float g = 0.f;
  if (pos >= 1 && pos + 1 < len) g -= 2.f * sgnf(diff2(dp, s)) * ds2_weight(imp, cs, step);
  if (pos >= 2) g += sgnf(diff2(dp - s, s)) * ds2_weight(imp - step, cs, step);
  if (pos + 2 < len) g += sgnf(diff2(dp + s, s)) * ds2_weight(imp + step, cs, step);
  return g;
}

template <bool MASK>
__global__ __launch_bounds__(256) void sss_fwd_tiles(const Work W, const Warps E) {
  __shared__ float reg[5][RW][RW + 1];
  __shared__ float hs[5][RW][T + 1];
  __shared__ float red[4][NPART];
  const int tile = blockIdx.x;
  const int i = find_item(W, tile);
  const dsm_selfsup_item& it = W.it[i];
  int b, ty0, tx0;
  tile_origin(W, i, tile, b, ty0, tx0);
  const Step P = step_scalars(W, i, E.delt1[i]);
  const int h = it.h, w = it.w;
  const long hw = (long)h * w;
  const float* disp = (const float*)it.disp + b * hw;
  const float* wp = E.warp[i] + b * 3L * hw;
  const float* imb = (const float*)it.im + (long)b * it.im_stride[0];
  const int cs = it.im_stride[1], ys = it.im_stride[2], xs = it.im_stride[3];

  for (int r = threadIdx.x; r < RW * RW; r += blockDim.x) {
    const int ry = r / RW, rx = r % RW;
    const int y = ty0 - HALO + ry, x = tx0 - HALO + rx;
    float m1 = 0.f, m2 = 0.f, q11 = 0.f, q22 = 0.f, q12 = 0.f;
    if (y >= 0 && y < h && x >= 0 && x < w) {
      float im[3], iw[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        im[c] = imb[(long)c * cs + (long)y * ys + (long)x * xs];
        iw[c] = wp[c * hw + (long)y * w + x];
      }
      m1 = (im[0] + im[1] + im[2]) / 3.f;
      m2 = (iw[0] + iw[1] + iw[2]) / 3.f;
      q11 = (im[0] * im[0] + im[1] * im[1] + im[2] * im[2]) / 3.f;
      q22 = (iw[0] * iw[0] + iw[1] * iw[1] + iw[2] * iw[2]) / 3.f;
      q12 = (im[0] * iw[0] + im[1] * iw[1] + im[2] * iw[2]) / 3.f;
    }
    reg[0][ry][rx] = m1; reg[1][ry][rx] = m2; reg[2][ry][rx] = q11; reg[3][ry][rx] = q22;
    reg[4][ry][rx] = q12;
  }
  __syncthreads();
  float st[5];
  filter_tile<5>(W, reg, hs, st);

  const int y = ty0 + threadIdx.x / T, x = tx0 + threadIdx.x % T;
  float part[NPART] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (y < h && x < w) {
    const long o = (long)y * w + x;
    const float d = disp[o];
    const float* imp = imb + (long)y * ys + (long)x * xs;
    const float mu1 = st[0], mu2 = st[1];
    const float A1 = 2.f * mu1 * mu2 + C1;
    const float A2 = 2.f * (st[4] - mu1 * mu2) + C2;
    const float B1 = mu1 * mu1 + mu2 * mu2 + C1;
    const float B2 = (st[2] - mu1 * mu1) + (st[3] - mu2 * mu2) + C2;
    const float inv = 1.f / (B1 * B2);
    const float S = A1 * A2 * inv;
    const Bil t = flip_taps(it, y, x, d);
    const float* wo = E.warp[i ^ 1] + b * 3L * hw;
    float ap = 3.f * 0.425f * (1.f - S), lr = 0.f, iw1_0 = 0.f;
    const bool valid = wp[o] != 0.f;                            // mask_ap (loss.py:288)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float im = imp[(long)c * cs], iw = wp[c * hw + o];
      float e = fabsf(im - iw);
      if (x + 1 < w) e += fabsf((imp[(long)c * cs + xs] - im) - (wp[c * hw + o + 1] - iw));      // C_imdiff1
      if (y + 1 < h) e += fabsf((imp[(long)c * cs + ys] - im) - (wp[c * hw + o + w] - iw));
      ap += 0.15f * e;
      float v, dv;
      bil_sample(wo + c * hw, w, 1, t, P.delt_im1, v, dv);
      if (c == 0) iw1_0 = v;
      lr += fabsf(im - v);
    }
    float wim = 1.f, wlr = 1.f;
    if (MASK) {
      const Pix q{&it, i, b, y, x, P.delt_im, P.delt_disp};
      float dw, ddw;
      disp_warp(q, d, dw, ddw);
      const float wc = weight_common(d, dw, it.scale_factor);
      wim = (iw1_0 == 0.f && valid) ? 1.f : wc;                 // loss.py:300-305
      wlr = (iw1_0 == 0.f) ? 0.f : wc;
    }
    float ds = 0.f;
    if (x >= 1 && x + 1 < w) ds += fabsf(diff2(disp + o, 1)) * ds2_weight(imp, cs, xs);
    if (y >= 1 && y + 1 < h) ds += fabsf(diff2(disp + o, w)) * ds2_weight(imp, cs, ys);
    part[0] = wim * ap;
    part[2] = ds;
    part[3] = wlr * lr;
    part[4] = valid ? S : 0.f;
    part[5] = valid ? 1.f : 0.f;
    part[6] = fabsf(d);
    const long n = (long)it.B * hw, p = b * hw + o;
    float* sv = W.save + W.save0[i];
    sv[p] = 2.f * mu1 * (A2 - A1) * inv - 2.f * mu2 * S * (1.f / B1 - 1.f / B2);      // dS / d mu2
    sv[n + p] = -S / B2;                                                              // dS / d E[y^2]
    sv[2 * n + p] = 2.f * A1 * inv;                                                   // dS / d E[xy]
    if (MASK) sv[3 * n + p] = wim;
  }
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll
  for (int k = 0; k < NPART; ++k) {
    const float s = wave_sum(part[k]);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < NPART) {
    const int k = threadIdx.x;
    W.part[(long)tile * NPART + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

// loss.py:287-292, 314-318: the mean over mask_ap however few pixels (none: w = 0.001, as Cap's
// rule), C = C_ap + C_ds w / 2^level + C_lr w + C_mdh 1e-4
__global__ __launch_bounds__(256) void sss_reduce(const Work W, float* loss, float* aux) {
  __shared__ double red[256];
  __shared__ double sums[DSM_SELFSUP_MAX_ITEMS][7];
  // the slab sums of selfsup_reduce, restated here so that that kernel keeps its instructions
  for (int i = 0; i < W.n; ++i) {
    for (int k = 0; k < 7; ++k) {
      double s = 0.0;
      for (int t = W.tile0[i] + threadIdx.x; t < W.tile0[i + 1]; t += blockDim.x)
        s += (double)W.part[(long)t * NPART + k];
      red[threadIdx.x] = s;
      __syncthreads();
      for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
      }
      if (threadIdx.x == 0) sums[i][k] = red[0];
      __syncthreads();
    }
  }
  if (threadIdx.x != 0) return;
  double total = 0.0;
  for (int j = 0; j < W.n; ++j) {
    const double n = (double)W.it[j].B * W.it[j].h * W.it[j].w;
    const bool any = sums[j][5] > 0.0;
    const double simlary = any ? sums[j][4] / sums[j][5] : 0.0;
    const double wt = any ? fmax(0.0, simlary - 0.75) / 2.0 + 0.001 : 0.001;
    const int dv = W.it[j].ds_divisor > 0 ? W.it[j].ds_divisor : 1;
    const double c = sums[j][0] / (3.0 * n) + (sums[j][2] / n) * (wt / (double)dv) +
                     (sums[j][3] / (3.0 * n)) * wt + (sums[j][6] / n) * 1e-4;
    aux[4 * j + 0] = (float)wt;
    aux[4 * j + 1] = 0.f;
    aux[4 * j + 2] = (float)c;
    aux[4 * j + 3] = (float)simlary;
    total += c * (double)item_weight(W, j);
  }
  loss[0] = (float)total;
}

template <bool MASK>
__global__ __launch_bounds__(256) void sss_bwd_tiles(const Work W, const Warps E, const float* __restrict__ aux,
                                                     const float* __restrict__ gloss) {
  __shared__ float reg[3][RW][RW + 1];
  __shared__ float hs[3][RW][T + 1];
  const int tile = blockIdx.x;
  const int i = find_item(W, tile);
  const dsm_selfsup_item& it = W.it[i];
  int b, ty0, tx0;
  tile_origin(W, i, tile, b, ty0, tx0);
  const Step P = step_scalars(W, i, E.delt1[i]);
  const int h = it.h, w = it.w;
  const long hw = (long)h * w, n = (long)it.B * hw;
  const float* sv = W.save + W.save0[i];
  const float* wimp = sv + 3 * n + b * hw;                    // weight_im of this sample (MASK only)
  const float wt = aux[4 * i + 0];
  const float wds = wt / (float)(it.ds_divisor > 0 ? it.ds_divisor : 1);
  const float gs = gloss[0] * P.weight;
  const float inv_n = 1.f / (float)n;
  const float* disp = (const float*)it.disp + b * hw;

  for (int r = threadIdx.x; r < RW * RW; r += blockDim.x) {
    const int ry = r / RW, rx = r % RW;
    const int y = ty0 - HALO + ry, x = tx0 - HALO + rx;
    float p0 = 0.f, p1 = 0.f, p2 = 0.f;
    if (y >= 0 && y < h && x >= 0 && x < w) {
      const long o = (long)y * w + x, p = b * hw + o;
      const float wim = MASK ? wimp[o] : 1.f;
      p0 = wim * sv[p]; p1 = wim * sv[n + p]; p2 = wim * sv[2 * n + p];
    }
    reg[0][ry][rx] = p0; reg[1][ry][rx] = p1; reg[2][ry][rx] = p2;
  }
  __syncthreads();
  float F[3];
  filter_tile<3>(W, reg, hs, F);

  const int y = ty0 + threadIdx.x / T, x = tx0 + threadIdx.x % T;
  if (y >= h || x >= w) return;
  const Pix q{&it, i, b, y, x, P.delt_im, P.delt_disp};
  const long o = (long)y * w + x;
  const float d = disp[o];
  float iw[3], div[3], im[3];
  image_warp(W, q, d, iw, div, im);
  const float* wp = E.warp[i] + b * 3L * hw;
  const float* imp = (const float*)it.im + (long)b * it.im_stride[0] + (long)y * it.im_stride[2] +
                     (long)x * it.im_stride[3];
  const int cs = it.im_stride[1], xs = it.im_stride[3], ys = it.im_stride[2];
  const float wim = MASK ? wimp[o] : 1.f;
  const float wimL = (MASK && x >= 1) ? wimp[o - 1] : 1.f, wimU = (MASK && y >= 1) ? wimp[o - w] : 1.f;

  // C_lr = |im - im_wrap1| weight_lr: the sample position (gather) and the sampled source (scatter)
  const Bil t = flip_taps(it, y, x, d);
  const float* wo = E.warp[i ^ 1] + b * 3L * hw;
  float v1[3], dv1[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) bil_sample(wo + c * hw, w, 1, t, P.delt_im1, v1[c], dv1[c]);
  float wlr = 1.f;
  if (MASK) {
    float dw, ddw;
    disp_warp(q, d, dw, ddw);
    wlr = (v1[0] == 0.f) ? 0.f : weight_common(d, dw, it.scale_factor);
  }

  float gix = 0.f, gd = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    // C_ap: the SSIM adjoint, the L1 sign, and C_imdiff1 -- im_wrap(p) ends the difference of p - 1
    // and starts the one of p, in x and in y
    const float imc = im[c], iwc = wp[c * hw + o];
    float e = wim * sgnf(iwc - imc);
    if (x + 1 < w) e -= wim * sgnf((wp[c * hw + o + 1] - iwc) - (imp[(long)c * cs + xs] - imc));
    if (x >= 1) e += wimL * sgnf((iwc - wp[c * hw + o - 1]) - (imc - imp[(long)c * cs - xs]));
    if (y + 1 < h) e -= wim * sgnf((wp[c * hw + o + w] - iwc) - (imp[(long)c * cs + ys] - imc));
    if (y >= 1) e += wimU * sgnf((iwc - wp[c * hw + o - w]) - (imc - imp[(long)c * cs - ys]));
    gix += ((-0.425f / 3.f) * inv_n * (F[0] + 2.f * iwc * F[1] + imc * F[2]) + (0.15f / 3.f) * inv_n * e) * div[c];
    const float s = sgnf(v1[c] - imc) * wlr * wt * inv_n / 3.f;
    gd += s * dv1[c] * ((float)w / (float)(w - 1));
    if (s != 0.f) {
      float* go = E.gwarp[i ^ 1] + (b * 3L + c) * hw;
      const float v = s * gs;
      if (t.in00) unsafeAtomicAdd(go + (long)t.y0 * w + t.x0, v * (t.wx0 * t.wy0));
      if (t.in01) unsafeAtomicAdd(go + (long)t.y0 * w + t.x0 + 1, v * (t.wx1 * t.wy0));
      if (t.in10) unsafeAtomicAdd(go + (long)(t.y0 + 1) * w + t.x0, v * (t.wx0 * t.wy1));
      if (t.in11) unsafeAtomicAdd(go + (long)(t.y0 + 1) * w + t.x0 + 1, v * (t.wx1 * t.wy1));
    }
  }
  gd += gix * (-(float)it.W0 / (float)(it.W0 - 1));
  gd += (ds2_bwd(disp + o, 1, x, w, imp, cs, xs) + ds2_bwd(disp + o, w, y, h, imp, cs, ys)) * wds * inv_n;
  gd += sgnf(d) * 1e-4f * inv_n;                               // C_mdh
  ((float*)it.grad_disp)[b * hw + o] = gd * gs;                // the element's first writer; sss_bwd_chain adds
}

// second stage: what the other view scattered into this item's d loss / d im_wrap, through
// d im_wrap / d ix (imwrap.py:67: dix/dd = -W0/(W0-1)), added by the pixel's own thread
__global__ __launch_bounds__(256) void sss_bwd_chain(const Work W, const Warps E) {
  const int tile = blockIdx.x;
  const int i = find_item(W, tile);
  const dsm_selfsup_item& it = W.it[i];
  int b, ty0, tx0;
  tile_origin(W, i, tile, b, ty0, tx0);
  const Step P = step_scalars(W, i, E.delt1[i]);
  const int y = ty0 + threadIdx.x / T, x = tx0 + threadIdx.x % T;
  if (y >= it.h || x >= it.w) return;
  const Pix q{&it, i, b, y, x, P.delt_im, P.delt_disp};
  const long hw = (long)it.h * it.w, o = (long)y * it.w + x;
  float iw[3], div[3], im[3];
  image_warp(W, q, ((const float*)it.disp)[b * hw + o], iw, div, im);
  float g = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) g += E.gwarp[i][(b * 3L + c) * hw + o] * div[c];
  ((float*)it.grad_disp)[b * hw + o] += g * (-(float)it.W0 / (float)(it.W0 - 1));
}

template <bool C, bool M, bool D, bool L>
struct Objective {
  static constexpr bool cap = C, mask = M, ds = D, lr = L;
};

// the flags word -> the kernel instantiation; false for a word that names no objective
template <class F>
bool with_objective(int flags, F&& f) {
  switch (flags) {
    case 0:
    case DSM_SELFSUP_MASK: f(Objective<false, false, true, true>{}); return true;     // depthmono[-mask]
#define DSM_CAP_CASE(M, D, L)                                                                   \
  case DSM_SELFSUP_CAP | (M ? DSM_SELFSUP_MASK : 0) | (D ? DSM_SELFSUP_DS : 0) | (L ? DSM_SELFSUP_LR : 0): \
    f(Objective<true, M, D, L>{});                                                              \
    return true;
    DSM_CAP_CASE(false, false, false) DSM_CAP_CASE(true, false, false)
    DSM_CAP_CASE(false, true, false) DSM_CAP_CASE(true, true, false)
    DSM_CAP_CASE(false, false, true) DSM_CAP_CASE(true, false, true)
    DSM_CAP_CASE(false, true, true) DSM_CAP_CASE(true, true, true)
#undef DSM_CAP_CASE
    default: return false;
  }
}

// the flags words of dsm_selfsup_ext_*: common[-mask], SsSMnet[-mask]
bool ext_objective(int flags) {
  const int o = flags & ~DSM_SELFSUP_MASK;
  return o == DSM_SELFSUP_COMMON || o == DSM_SELFSUP_SSSMNET;
}

// the side array of SsSMnet; the backward needs the scatter buffers too
int make_warps(const dsm_selfsup_ext* ext, int n, bool bwd, Warps& E) {
  DSM_REQUIRE(ext, DSM_ERR_ARG);
  for (int i = 0; i < n; ++i) {
    DSM_REQUIRE(ext[i].warp && (ext[i].grad_warp || !bwd), DSM_ERR_ARG);
    E.warp[i] = (float*)ext[i].warp;
    E.gwarp[i] = (float*)ext[i].grad_warp;
    E.delt1[i] = ext[i].delt_im1;
  }
  return DSM_OK;
}

int make_work(const dsm_selfsup_item* items, int n, int flags, void* workspace, Work& W, bool ext = false,
              const float* params = nullptr) {
  DSM_REQUIRE(items && workspace, DSM_ERR_ARG);
  DSM_REQUIRE(n >= 2 && n <= DSM_SELFSUP_MAX_ITEMS && n % 2 == 0, DSM_ERR_ARG);
  DSM_REQUIRE(ext ? ext_objective(flags) : with_objective(flags, [](auto) {}), DSM_ERR_ARG);
  W.n = n;
  W.flag_mask = flags & DSM_SELFSUP_MASK;
  W.cap = (flags & DSM_SELFSUP_CAP) != 0;
  W.ds = !W.cap || (flags & DSM_SELFSUP_DS);
  W.lr = !W.cap || (flags & DSM_SELFSUP_LR);
  W.gm_B = 0;
  long tiles = 0, save = 0;
  for (int i = 0; i < n; ++i) {
    const dsm_selfsup_item& it = items[i];
    if (ext) DSM_REQUIRE(3L * it.h * it.w < (1L << 31), DSM_ERR_UNSUPPORTED);   // common_gradmean's index
    W.gm_B = it.B > W.gm_B ? it.B : W.gm_B;
    DSM_REQUIRE(it.im && it.src && it.disp && it.disp_other, DSM_ERR_ARG);
    DSM_REQUIRE(it.B > 0 && it.h > 1 && it.w > 1 && it.H0 > 1 && it.W0 > 1, DSM_ERR_ARG);   // imwrap.py:48
    DSM_REQUIRE(it.scale_factor > 0 && it.left >= 0 && it.top >= 0 && it.ds_divisor >= 0, DSM_ERR_ARG);
    if (i % 2 == 1) DSM_REQUIRE(it.B == items[i - 1].B && it.h == items[i - 1].h && it.w == items[i - 1].w, DSM_ERR_ARG);
    W.it[i] = it;
    W.ntx[i] = dsm_cdiv(it.w, T);
    W.nty[i] = dsm_cdiv(it.h, T);
    W.tile0[i] = (int)tiles;
    W.save0[i] = save;
    tiles += (long)it.B * W.ntx[i] * W.nty[i];
    save += (long)NSAVE * it.B * it.h * it.w;
    DSM_REQUIRE(tiles < (1L << 30), DSM_ERR_UNSUPPORTED);
    // imwrap.py:51-54, in double as the reference's Python does; torch.linspace takes them as fp32
    const double x = it.left * 2.0 / (it.W0 - 1) - 1.0, y = it.top * 2.0 / (it.H0 - 1) - 1.0;
    W.xs[i] = (float)x;
    W.xe[i] = (float)(x + (it.w - 1) * (double)it.scale_factor * 2.0 / (it.W0 - 1));
    W.ys[i] = (float)y;
    W.ye[i] = (float)(y + (it.h - 1) * (double)it.scale_factor * 2.0 / (it.H0 - 1));
  }
  W.tile0[n] = (int)tiles;
  float gf[11], sumf = 0.f;                       // SSIM.py:6-8 (torch normalises in fp32)
  double sumd = 0.0;
  for (int k = 0; k < 11; ++k) {
    gf[k] = (float)exp(-(k - 5) * (k - 5) / (2.0 * 1.5 * 1.5));
    sumf += gf[k];
    sumd += gf[k];
  }
  // torch's fp32 g.sum() is a vectorised sum and lands on the correctly rounded value, one ulp above
  // this sequential one: the two windows then sum to 1 - 6.9e-8 and 1 + 8.9e-8, which
  // E[x^2] - mu^2 turns into a one-sided 4e-8 on variances of ~1e-3 and so into a one-sided ~2e-6
  // on simlary.  Cap's w = (simlary - 0.75) / 2 + 0.001 amplifies that, so Cap takes torch's taps;
  // depthmono keeps the sequential sum and with it the bits it always gave; common has no bits
  // to keep and takes torch's too
  if (W.cap || ext) sumf = (float)sumd;
  for (int k = 0; k < 11; ++k) W.g[k] = gf[k] / sumf;
  W.part = (float*)workspace;
  W.save = W.part + tiles * NPART;
  W.gmean = W.save + save;
  W.params = params;
  return DSM_OK;
}

// dsm_selfsup_dyn_*: the array is there and step_scalars' float4 load is aligned
int check_params(const float* params) {
  DSM_REQUIRE(params, DSM_ERR_ARG);
  DSM_REQUIRE(dsm_aligned16(params), DSM_ERR_ALIGN);
  return DSM_OK;
}

int fwd(const dsm_selfsup_item* items, int n_items, int flags, const float* params, void* workspace,
        void* loss, void* aux, dsm_stream_t stream) {
  DSM_REQUIRE(loss && aux, DSM_ERR_ARG);
  Work W;
  const int rc = make_work(items, n_items, flags, workspace, W, false, params);
  if (rc != DSM_OK) return rc;
  dsm_clear_stale_error();
  with_objective(flags, [&](auto o) {
    using O = decltype(o);
    hipLaunchKernelGGL((selfsup_fwd_tiles<O::cap, O::mask, O::ds, O::lr>), dim3(W.tile0[W.n]), dim3(256), 0,
                       (hipStream_t)stream, W);
  });
  hipLaunchKernelGGL(selfsup_reduce, dim3(1), dim3(256), 0, (hipStream_t)stream, W, (float*)loss,
                     (float*)aux);
  return dsm_launch_status();
}

int bwd(const dsm_selfsup_item* items, int n_items, int flags, const float* params, const void* workspace,
        const void* aux, const void* grad_loss, dsm_stream_t stream) {
  DSM_REQUIRE(aux && grad_loss, DSM_ERR_ARG);
  // Cap without the lr term: nothing scatters into the other view, grad_other is not needed
  const bool gather_only = (flags & DSM_SELFSUP_CAP) && !(flags & DSM_SELFSUP_LR);
  for (int i = 0; items && i < n_items && i < DSM_SELFSUP_MAX_ITEMS; ++i)
    DSM_REQUIRE(items[i].grad_disp && (items[i].grad_other || gather_only), DSM_ERR_ARG);
  Work W;
  const int rc = make_work(items, n_items, flags, (void*)workspace, W, false, params);
  if (rc != DSM_OK) return rc;
  dsm_clear_stale_error();
  with_objective(flags, [&](auto o) {
    using O = decltype(o);
    hipLaunchKernelGGL((selfsup_bwd_tiles<O::cap, O::mask, O::ds, O::lr>), dim3(W.tile0[W.n]), dim3(256), 0,
                       (hipStream_t)stream, W, (const float*)aux, (const float*)grad_loss);
  });
  return dsm_launch_status();
}

int ext_fwd(const dsm_selfsup_item* items, const dsm_selfsup_ext* ext, int n_items, int flags,
            const float* params, void* workspace, void* loss, void* aux, dsm_stream_t stream) {
  DSM_REQUIRE(loss && aux, DSM_ERR_ARG);
  Work W;
  int rc = make_work(items, n_items, flags, workspace, W, true, params);
  if (rc != DSM_OK) return rc;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 tiles(W.tile0[W.n]), block(256);
  if (flags & DSM_SELFSUP_SSSMNET) {
    Warps E;
    if ((rc = make_warps(ext, n_items, false, E)) != DSM_OK) return rc;
    dsm_clear_stale_error();
    hipLaunchKernelGGL(sss_warp, tiles, block, 0, st, W, E);
    if (W.flag_mask) hipLaunchKernelGGL(sss_fwd_tiles<true>, tiles, block, 0, st, W, E);
    else hipLaunchKernelGGL(sss_fwd_tiles<false>, tiles, block, 0, st, W, E);
    hipLaunchKernelGGL(sss_reduce, dim3(1), block, 0, st, W, (float*)loss, (float*)aux);
    return dsm_launch_status();
  }
  dsm_clear_stale_error();
  hipLaunchKernelGGL(common_gradmean, dim3(NCH, W.gm_B, W.n), block, 0, st, W);
  hipLaunchKernelGGL((selfsup_fwd_tiles<false, false, true, true, true>), tiles, block, 0, st, W);
  hipLaunchKernelGGL(selfsup_reduce, dim3(1), block, 0, st, W, (float*)loss, (float*)aux);
  return dsm_launch_status();
}

int ext_bwd(const dsm_selfsup_item* items, const dsm_selfsup_ext* ext, int n_items, int flags,
            const float* params, const void* workspace, const void* aux, const void* grad_loss,
            dsm_stream_t stream) {
  DSM_REQUIRE(aux && grad_loss, DSM_ERR_ARG);
  const bool sss = (flags & DSM_SELFSUP_SSSMNET) != 0;        // SsSMnet scatters into grad_warp, not grad_other
  for (int i = 0; items && i < n_items && i < DSM_SELFSUP_MAX_ITEMS; ++i)
    DSM_REQUIRE(items[i].grad_disp && (items[i].grad_other || sss), DSM_ERR_ARG);
  Work W;
  int rc = make_work(items, n_items, flags, (void*)workspace, W, true, params);
  if (rc != DSM_OK) return rc;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 tiles(W.tile0[W.n]), block(256);
  if (sss) {
    Warps E;
    if ((rc = make_warps(ext, n_items, true, E)) != DSM_OK) return rc;
    dsm_clear_stale_error();
    if (W.flag_mask)
      hipLaunchKernelGGL(sss_bwd_tiles<true>, tiles, block, 0, st, W, E, (const float*)aux, (const float*)grad_loss);
    else
      hipLaunchKernelGGL(sss_bwd_tiles<false>, tiles, block, 0, st, W, E, (const float*)aux, (const float*)grad_loss);
    hipLaunchKernelGGL(sss_bwd_chain, tiles, block, 0, st, W, E);
    return dsm_launch_status();
  }
  dsm_clear_stale_error();
  hipLaunchKernelGGL((selfsup_bwd_tiles<false, false, true, true, true>), tiles, block, 0, st, W,
                     (const float*)aux, (const float*)grad_loss);
  return dsm_launch_status();
}

}  // namespace

extern "C" size_t dsm_selfsup_workspace_floats(const dsm_selfsup_item* items, int n_items) {
  if (!items || n_items < 1 || n_items > DSM_SELFSUP_MAX_ITEMS) return 0;
  size_t f = 0;
  for (int i = 0; i < n_items; ++i) {
    const dsm_selfsup_item& it = items[i];
    if (it.B <= 0 || it.h <= 0 || it.w <= 0) return 0;
    f += (size_t)it.B * dsm_cdiv(it.w, T) * dsm_cdiv(it.h, T) * NPART + (size_t)NSAVE * it.B * it.h * it.w;
  }
  return f;
}

extern "C" int dsm_selfsup_fwd(const dsm_selfsup_item* items, int n_items, int flags, void* workspace,
                               void* loss, void* aux, dsm_stream_t stream) {
  return fwd(items, n_items, flags, nullptr, workspace, loss, aux, stream);
}

extern "C" int dsm_selfsup_bwd(const dsm_selfsup_item* items, int n_items, int flags,
                               const void* workspace, const void* aux, const void* grad_loss,
                               dsm_stream_t stream) {
  return bwd(items, n_items, flags, nullptr, workspace, aux, grad_loss, stream);
}

// ---- common[-mask] and SsSMnet[-mask]: the entry points that take the objectives
// dsm_selfsup_fwd's flags word refuses

extern "C" size_t dsm_selfsup_ext_workspace_floats(const dsm_selfsup_item* items, int n_items, int flags) {
  const size_t f = dsm_selfsup_workspace_floats(items, n_items);
  if (f == 0 || !ext_objective(flags)) return 0;
  int B = 0;
  for (int i = 0; i < n_items; ++i) B = items[i].B > B ? items[i].B : B;
  return f + (size_t)n_items * B * NCH * 2;
}

extern "C" int dsm_selfsup_ext_fwd(const dsm_selfsup_item* items, const dsm_selfsup_ext* ext, int n_items,
                                   int flags, void* workspace, void* loss, void* aux, dsm_stream_t stream) {
  return ext_fwd(items, ext, n_items, flags, nullptr, workspace, loss, aux, stream);
}

extern "C" int dsm_selfsup_ext_bwd(const dsm_selfsup_item* items, const dsm_selfsup_ext* ext, int n_items,
                                   int flags, const void* workspace, const void* aux, const void* grad_loss,
                                   dsm_stream_t stream) {
  return ext_bwd(items, ext, n_items, flags, nullptr, workspace, aux, grad_loss, stream);
}

// ---- the per-step scalars from device memory: every flags word of the entry points above, the same
// kernels, `params` read when they run

extern "C" int dsm_selfsup_dyn_fwd(const dsm_selfsup_item* items, const dsm_selfsup_ext* ext, int n_items,
                                   int flags, const float* params, void* workspace, void* loss, void* aux,
                                   dsm_stream_t stream) {
  const int rc = check_params(params);
  if (rc != DSM_OK) return rc;
  return ext_objective(flags) ? ext_fwd(items, ext, n_items, flags, params, workspace, loss, aux, stream)
                              : fwd(items, n_items, flags, params, workspace, loss, aux, stream);
}

extern "C" int dsm_selfsup_dyn_bwd(const dsm_selfsup_item* items, const dsm_selfsup_ext* ext, int n_items,
                                   int flags, const float* params, const void* workspace, const void* aux,
                                   const void* grad_loss, dsm_stream_t stream) {
  const int rc = check_params(params);
  if (rc != DSM_OK) return rc;
  return ext_objective(flags) ? ext_bwd(items, ext, n_items, flags, params, workspace, aux, grad_loss, stream)
                              : bwd(items, n_items, flags, params, workspace, aux, grad_loss, stream);
}
