// Evaluation metrics of a disparity map, fused (utils/evaluate.py:9-73 evaluate, imwrap_pixel_errors,
// compute_errors; stereo.py:103-113 accuracy; utils/imwrap.py:37-72 imwrap_BCHW at LeftTop [0,0], scale 1).
//
// Stock torch spends about 40 launches and several host reads per batch on these (boolean gathers, one
// mean per metric, linspace grids, grid_sample, masks).  Everything is a reduction over the same pixels
// plus one bilinear gather, so here it is one pass and one fixed-order reduction, no host read:
//   metrics_tiles    per (image, 16x64 tile): pred, gt and imL read once (16 bytes per lane where the
//                    rows allow it), the warped right image sampled per channel, 16 sums per tile to a
//                    float64 slab row with plain stores
//   metrics_reduce   one workgroup per image: its slab rows summed in a fixed order (fp64) to out[b][16]
// No atomics anywhere: two runs give the same bits.
//
// Slab row (m = gt > 0, diff = |gt - pred|; per-element arithmetic in fp32, plain `/`, fp32 thresholds):
//   0  count m                         8, 9, 10  count max(gt / (pred + 1e-6), pred / gt) < 1.25^1,2,3
//   1  sum diff                        11, 12    count and sum |imL - w| over elements with w > 0
//   2  count diff <= 3 or diff/gt <= 0.05        (imwrap_pixel_errors, evaluate.py:42-43)
//   3  count diff >= 3 and diff/gt >= 0.05       13, 14  pixels whose channel sum of w is > 0, and
//   4  sum diff^2                                sum |imL - w| over all C channels of those pixels
//   5  sum (ln gt - ln(pred + 1e-6))^2           (evaluate.py:27-29, read as the broadcast it means)
//   6  sum diff / gt                   15        sum |imL - w| over every element (evaluate.py:30)
//   7  sum diff^2 / gt
// w = imwrap_BCHW(imR, +-pred) with the arithmetic of warp_abs_error_kernel (common.hpp,
// dsm_warp_taps_at / dsm_warp_sample).  Slots of an absent input are written as 0.
#include "common.hpp"

namespace {

constexpr int TH = 16, TW = 64;            // tile: 1024 pixels, four consecutive columns per thread
constexpr int NS = DSM_METRICS_SLOTS;
static_assert(sizeof(dsm_metrics_args) == 72, "dsm_metrics_args layout (ctypes mirror in _lib.py)");

struct Work {
  const float* pred;
  const float* gt;
  const float* imL;
  const float* imR;
  double* part;                            // [b][tile][NS]
  double* out;                             // [b][NS]
  int B, C, H, W, nty, ntx, per;           // per = tiles of one image
  int vec;                                 // 16-byte loads of pred, gt and imL
  float delt, sign;
};

__device__ __forceinline__ void load4(const float* row, int x, int W, bool vec, float v[4]) {
  if (vec) {                               // W % 4 == 0: the four pixels are inside together
    const f32x4 q = *(const f32x4*)(row + x);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = x + k < W ? row[x + k] : 0.f;
  }
}

__global__ __launch_bounds__(256) void metrics_tiles(const Work K) {
  __shared__ double red[4][NS];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / K.per, local = blockIdx.x - b * K.per;
  const int H = K.H, W = K.W, C = K.C;
  const int y = (local / K.ntx) * TH + tid / (TW / 4);
  const int x = (local % K.ntx) * TW + (tid % (TW / 4)) * 4;
  const bool in = y < H && x < W;
  const long plane = (long)H * W;
  const long o = (long)b * plane + (long)y * W;        // the pixel row in a one-channel map
  float s[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) s[k] = 0.f;

  if (in) {
    float p[4], g[4];
    load4(K.pred + o, x, W, K.vec, p);
    if (K.gt) {
      load4(K.gt + o, x, W, K.vec, g);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (x + k >= W || !(g[k] > 0.f)) continue;
        const float diff = fabsf(g[k] - p[k]), rel = diff / g[k], sq = diff * diff;
        const float pe = p[k] + 1e-6f;
        const float lg = logf(g[k]) - logf(pe);
        const float th = fmaxf(g[k] / pe, p[k] / g[k]);
        s[0] += 1.f;
        s[1] += diff;
        s[2] += (diff <= 3.f || rel <= 0.05f) ? 1.f : 0.f;
        s[3] += (diff >= 3.f && rel >= 0.05f) ? 1.f : 0.f;
        s[4] += sq;
        s[5] += lg * lg;
        s[6] += rel;
        s[7] += sq / g[k];
        s[8] += th < 1.25f ? 1.f : 0.f;
        s[9] += th < 1.5625f ? 1.f : 0.f;
        s[10] += th < 1.953125f ? 1.f : 0.f;
      }
    }
    if (K.imL) {
      dsm_warp_taps T[4];
      long ro[4];
      float wsum[4] = {0.f, 0.f, 0.f, 0.f}, asum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        // the base grid of a map as large as the image ends at 1: x1 = y1 = 1 exactly
        T[k] = dsm_warp_taps_at(K.sign * p[k], min(x + k, W - 1), y, H, W, H, W, 1.f, 1.f);
        ro[k] = (long)T[k].y0 * W + T[k].x0;           // dereferenced behind i00..i11 only
      }
      for (int c = 0; c < C; ++c) {
        const long oc = ((long)b * C + c) * plane;
        float l[4];
        load4(K.imL + oc + (long)y * W, x, W, K.vec, l);
        const float* r = K.imR + oc;
        float t[4][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {                  // the sixteen taps in flight together
          t[k][0] = T[k].i00 ? r[ro[k]] : 0.f;
          t[k][1] = T[k].i01 ? r[ro[k] + 1] : 0.f;
          t[k][2] = T[k].i10 ? r[ro[k] + W] : 0.f;
          t[k][3] = T[k].i11 ? r[ro[k] + W + 1] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (x + k >= W) continue;
          const float w = dsm_warp_sample(T[k], t[k][0], t[k][1], t[k][2], t[k][3], K.delt);
          const float ad = fabsf(l[k] - w);
          if (w > 0.f) {
            s[11] += 1.f;
            s[12] += ad;
          }
          s[15] += ad;
          wsum[k] += w;
          asum[k] += ad;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (x + k < W && wsum[k] > 0.f) {
          s[13] += 1.f;
          s[14] += asum[k];
        }
    }
  }

  // fixed order: per thread (above), the wave's 64 lanes, then four LDS slots
  const int wave = tid / 64, lane = tid % 64;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    double v = (double)s[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (tid < NS)
    K.part[(long)blockIdx.x * NS + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// one workgroup per image: thread (j, slot) sums rows j, j + 16, ... of its slot, then the sixteen
// partial sums of a slot are added in the order of j
__global__ __launch_bounds__(256) void metrics_reduce(const Work K) {
  __shared__ double red[16][NS];
  const int tid = threadIdx.x, slot = tid % NS, j = tid / NS;
  const double* slab = K.part + (long)blockIdx.x * K.per * NS;
  double v = 0.0;
  for (int t = j; t < K.per; t += 16) v += slab[(long)t * NS + slot];
  red[j][slot] = v;
  __syncthreads();
  if (tid < NS) {
    double a = red[0][tid];
#pragma unroll
    for (int q = 1; q < 16; ++q) a += red[q][tid];
    K.out[(long)blockIdx.x * NS + tid] = a;
  }
}

}  // namespace

extern "C" size_t dsm_stereo_metrics_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)B * dsm_cdiv(H, TH) * dsm_cdiv(W, TW) * NS * sizeof(double);
}

extern "C" int dsm_stereo_metrics(const dsm_metrics_args* a, dsm_stream_t stream) {
  DSM_REQUIRE(a && a->pred && a->out && a->workspace, DSM_ERR_ARG);
  DSM_REQUIRE((a->imL != nullptr) == (a->imR != nullptr), DSM_ERR_ARG);
  DSM_REQUIRE(a->gt || a->imL, DSM_ERR_ARG);
  DSM_REQUIRE(a->B > 0 && a->C > 0 && a->H > 0 && a->W > 0, DSM_ERR_ARG);
  DSM_REQUIRE(!a->imL || (a->H > 1 && a->W > 1), DSM_ERR_ARG);       // imwrap.py:48
  DSM_REQUIRE(a->flags == 0 || a->flags == DSM_METRICS_NEGATE_WARP, DSM_ERR_ARG);
  const uintptr_t maps = (uintptr_t)a->pred | (uintptr_t)a->gt | (uintptr_t)a->imL | (uintptr_t)a->imR;
  DSM_REQUIRE((maps & 3u) == 0, DSM_ERR_ALIGN);
  DSM_REQUIRE((((uintptr_t)a->workspace | (uintptr_t)a->out) & 7u) == 0, DSM_ERR_ALIGN);
  Work K;
  K.B = a->B; K.C = a->C; K.H = a->H; K.W = a->W;
  K.nty = dsm_cdiv(a->H, TH); K.ntx = dsm_cdiv(a->W, TW);
  const long per = (long)K.nty * K.ntx;
  DSM_REQUIRE(per * a->B < (1L << 31), DSM_ERR_UNSUPPORTED);          // the grid's x extent
  K.per = (int)per;
  K.pred = (const float*)a->pred; K.gt = (const float*)a->gt;
  K.imL = (const float*)a->imL; K.imR = (const float*)a->imR;
  K.part = (double*)a->workspace; K.out = (double*)a->out;
  K.vec = (a->W % 4 == 0 && dsm_aligned16(a->pred) && (!a->gt || dsm_aligned16(a->gt)) &&
           (!a->imL || dsm_aligned16(a->imL))) ? 1 : 0;
  K.delt = a->delt;
  K.sign = (a->flags & DSM_METRICS_NEGATE_WARP) ? -1.f : 1.f;
  dsm_clear_stale_error();
  hipLaunchKernelGGL(metrics_tiles, dim3((unsigned)(per * a->B)), dim3(256), 0, (hipStream_t)stream, K);
  hipLaunchKernelGGL(metrics_reduce, dim3(a->B), dim3(256), 0, (hipStream_t)stream, K);
  return dsm_launch_status();
}
