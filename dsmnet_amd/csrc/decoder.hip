// One decoder level of DispNetC / iResNet in one launch -- models/dispnetcorr.py:89-132 and
// models/iresnet.py:119-161,186-193:
//     myCat2d( relu(deconv(x) + bias),  upsample(pr),  skip )
// where the reference runs ConvTranspose2d (+ bias) -> ReLU -> nn.Upsample(scale_factor=2,
// bilinear) -> three crops to the common (h, w) (util_fun.py:7-15) -> torch.cat: ~7 launches per
// level and 5-6 levels per forward (~65 element-wise launches, 0.4 of DispNetC's 2.3 ms).
// Here the transposed convolution runs WITHOUT its bias (stock kernel) and this kernel does the
// rest: out (B, Cu + Cp + Cs, h, w) NCHW fp32, h = min(Hu, 2 Hp, Hs), w likewise.
//   channels [0, Cu):        relu?(up + bias[c])            (bit-identical to the stock ops)
//   channels [Cu, Cu + Cp):  bilinear x2 of pr, align_corners = False, with torch's
//                            area_pixel_compute_source_index arithmetic (scale 0.5)
//   channels [Cu + Cp, ...): skip
// HBM-bound streaming copy; each thread moves 4 consecutive x.
#include "common.hpp"

namespace {

struct DecCatParams {
  const float* up; const float* bias; const float* pr; const float* skip; float* out;
  int B, Cu, Cp, Cs;
  int Hu, Wu, Hp, Wp, Hs, Ws;
  int h, w, relu;
};

__device__ __forceinline__ float up2_sample(const float* __restrict__ plane, int Hp, int Wp, int y, int x) {
  const float sy = fmaxf(0.5f * (y + 0.5f) - 0.5f, 0.f), sx = fmaxf(0.5f * (x + 0.5f) - 0.5f, 0.f);
  const int y0 = (int)sy, x0 = (int)sx;
  const int y1 = y0 + (y0 < Hp - 1 ? 1 : 0), x1 = x0 + (x0 < Wp - 1 ? 1 : 0);
  const float ly = sy - y0, lx = sx - x0;
  const float hy = 1.f - ly, hx = 1.f - lx;
  return hy * (hx * plane[y0 * Wp + x0] + lx * plane[y0 * Wp + x1]) +
         ly * (hx * plane[y1 * Wp + x0] + lx * plane[y1 * Wp + x1]);
}

__global__ __launch_bounds__(256) void decoder_cat_kernel(DecCatParams p) {
  const int wq = (p.w + 3) >> 2;
  const int C = p.Cu + p.Cp + p.Cs;
  const long n = (long)p.B * C * p.h * wq;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  long t = i;
  const int xq = t % wq; t /= wq;
  const int y = t % p.h; t /= p.h;
  const int c = t % C; const int b = t / C;
  const int x0 = 4 * xq;
  float v[4];
  if (c < p.Cu) {
    const float* src = p.up + (((long)b * p.Cu + c) * p.Hu + y) * p.Wu;
    const float bs = p.bias ? p.bias[c] : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float a = (x0 + k < p.w) ? src[x0 + k] + bs : 0.f;
      v[k] = p.relu ? fmaxf(a, 0.f) : a;
    }
  } else if (c < p.Cu + p.Cp) {
    const float* plane = p.pr + ((long)b * p.Cp + (c - p.Cu)) * p.Hp * p.Wp;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (x0 + k < p.w) ? up2_sample(plane, p.Hp, p.Wp, y, x0 + k) : 0.f;
  } else {
    const float* src = p.skip + (((long)b * p.Cs + (c - p.Cu - p.Cp)) * p.Hs + y) * p.Ws;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (x0 + k < p.w) ? src[x0 + k] : 0.f;
  }
  float* dst = p.out + (((long)b * C + c) * p.h + y) * p.w + x0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (x0 + k < p.w) dst[k] = v[k];
}

// Backward of decoder_cat_kernel (training: the same decoder levels under autograd).  g and out are
// (B, Cu + Cp + Cs, h, w); out is the forward's result, whose first Cu channels carry the ReLU mask.
//   g_up   (B,Cu,Hu,Wu) = g[:, :Cu] * (out > 0), zero in the cropped-off rows / columns
//   g_bias (Cu)         = sum of g_up over (b, y, x): block sums, one fp32 atomic per block
//   g_skip (B,Cs,Hs,Ws) = g[:, Cu+Cp:], zero-padded likewise
//   g_pr   (B,Cp,Hp,Wp) = the adjoint of up2_sample over the h x w crop, gathered: a pr element is touched by
//                         output rows 2 py - 2 .. 2 py + 2 at most (and columns likewise); each candidate's
//                         y0 / y1 / ly / hy are recomputed with the forward's expressions, clamps included
// Block ranges of the 1-D grid: [0, nbu) g_up, [nbu, nbu + nbs) g_skip, the rest g_pr.  A copy block
// moves DEC_ITER x 256 quads of 4 consecutive x of ONE (b, c) plane, so its bias sum has one destination.
struct DecBwdParams {
  const float* g; const float* out; float* g_up; float* g_bias; float* g_pr; float* g_skip;
  int B, Cu, Cp, Cs;
  int Hu, Wu, Hp, Wp, Hs, Ws;
  int h, w, relu;
  int cbu, cbs;            // copy blocks per plane of g_up / g_skip
  long nbu, nbs;           // blocks of the two copy ranges
};

constexpr int DEC_ITER = 4;

// rows of `dst` plane (Hd x Wd) <- the h x w crop of g's plane (times the mask), zeros elsewhere
__device__ __forceinline__ float dec_copy_block(const DecBwdParams& p, const float* __restrict__ gpl,
                                                const float* __restrict__ mpl, float* __restrict__ dpl,
                                                int Hd, int Wd, int chunk) {
  const int wq = (Wd + 3) >> 2;
  const long nq = (long)Hd * wq;
  float acc = 0.f;
#pragma unroll
  for (int it = 0; it < DEC_ITER; ++it) {
    const long q = ((long)chunk * DEC_ITER + it) * 256 + threadIdx.x;
    if (q >= nq) break;
    const int y = (int)(q / wq), x0 = 4 * (int)(q % wq);
    float v[4], m[4];
    const long so = (long)y * p.w + x0;
    if (y < p.h && x0 + 3 < p.w) {                  // w <= Wd; rows of g are only dword-aligned
      const f32x4u gq = *reinterpret_cast<const f32x4u*>(gpl + so);
      const f32x4u mq = mpl ? *reinterpret_cast<const f32x4u*>(mpl + so) : f32x4u{1.f, 1.f, 1.f, 1.f};
#pragma unroll
      for (int k = 0; k < 4; ++k) { v[k] = gq[k]; m[k] = mq[k]; }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool in = y < p.h && x0 + k < p.w;
        v[k] = in ? gpl[so + k] : 0.f;
        m[k] = (in && mpl) ? mpl[so + k] : 1.f;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k] = m[k] > 0.f ? v[k] : 0.f;
      acc += v[k];
    }
    if (dpl) {
      float* dst = dpl + (long)y * Wd + x0;
      if (x0 + 3 < Wd) {
        *reinterpret_cast<f32x4u*>(dst) = f32x4u{v[0], v[1], v[2], v[3]};
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (x0 + k < Wd) dst[k] = v[k];
      }
    }
  }
  return acc;
}

__global__ __launch_bounds__(256) void decoder_cat_bwd_kernel(DecBwdParams p) {
  __shared__ float wsum[4];
  const int C = p.Cu + p.Cp + p.Cs;
  const long hw = (long)p.h * p.w;
  const long blk = blockIdx.x;
  if (blk < p.nbu) {
    const long pl = blk / p.cbu; const int chunk = (int)(blk % p.cbu);
    const int c = (int)(pl % p.Cu); const long b = pl / p.Cu;
    const long src = (b * C + c) * hw;
    float acc = dec_copy_block(p, p.g + src, p.relu ? p.out + src : nullptr,
                               p.g_up ? p.g_up + pl * p.Hu * p.Wu : nullptr, p.Hu, p.Wu, chunk);
    if (!p.g_bias) return;                          // uniform over the block
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) unsafeAtomicAdd(p.g_bias + c, (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]));
    return;
  }
  if (blk < p.nbu + p.nbs) {
    const long r = blk - p.nbu;
    const long pl = r / p.cbs; const int chunk = (int)(r % p.cbs);
    const int c = (int)(pl % p.Cs); const long b = pl / p.Cs;
    dec_copy_block(p, p.g + (b * C + p.Cu + p.Cp + c) * hw, nullptr, p.g_skip + pl * p.Hs * p.Ws,
                   p.Hs, p.Ws, chunk);
    return;
  }
  const long i = (blk - p.nbu - p.nbs) * 256 + threadIdx.x;
  if (i >= (long)p.B * p.Cp * p.Hp * p.Wp) return;
  const int px = (int)(i % p.Wp), py = (int)((i / p.Wp) % p.Hp);
  const long pl = i / ((long)p.Wp * p.Hp);
  const int c = (int)(pl % p.Cp); const long b = pl / p.Cp;
  const float* gpl = p.g + (b * C + p.Cu + c) * hw;
  float wy[5], wx[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {                     // weight of output row / column 2 p - 2 + k on this element
    const int y = 2 * py - 2 + k, x = 2 * px - 2 + k;
    wy[k] = wx[k] = 0.f;
    if (y >= 0 && y < p.h) {
      const float sy = fmaxf(0.5f * (y + 0.5f) - 0.5f, 0.f);
      const int y0 = (int)sy, y1 = y0 + (y0 < p.Hp - 1 ? 1 : 0);
      const float ly = sy - y0, hy = 1.f - ly;
      wy[k] = (y0 == py ? hy : 0.f) + (y1 == py ? ly : 0.f);
    }
    if (x >= 0 && x < p.w) {
      const float sx = fmaxf(0.5f * (x + 0.5f) - 0.5f, 0.f);
      const int xx0 = (int)sx, xx1 = xx0 + (xx0 < p.Wp - 1 ? 1 : 0);
      const float lx = sx - xx0, hx = 1.f - lx;
      wx[k] = (xx0 == px ? hx : 0.f) + (xx1 == px ? lx : 0.f);
    }
  }
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int y = 2 * py - 2 + j;
    if (wy[j] == 0.f) continue;                     // also every y outside [0, h)
    float row = 0.f;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int x = 2 * px - 2 + k;
      if (wx[k] != 0.f) row += wx[k] * gpl[(long)y * p.w + x];
    }
    acc += wy[j] * row;
  }
  p.g_pr[i] = acc;
}

__global__ __launch_bounds__(256) void decoder_zero_kernel(float* __restrict__ p, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = 0.f;
}

// Image staging of the 2-D towers: the two views (B,C,H,W) NCHW, C <= 16, become ONE batch
// (2B,16,H,W) in NHWC memory with zero channels C..15 -- the 16-channel granularity the MFMA kernel
// stages.  One pass instead of torch.cat + two strided copies + a fill (4-5 launches, 66 us at
// 384 x 1280).  `right` may be NULL (one view: B images).  Thread = one pixel: C coalesced plane
// reads, four 16-byte stores.
__global__ __launch_bounds__(256) void stage_pair_kernel(const float* __restrict__ left,
                                                         const float* __restrict__ right,
                                                         float* __restrict__ out, int B, int C, long hw) {
  const long n = (long)(right ? 2 * B : B) * hw;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long b = i / hw, px = i % hw;
  const float* src = (b < B ? left + b * C * hw : right + (b - B) * C * hw) + px;
  float v[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) v[c] = c < C ? src[c * hw] : 0.f;
  f32x4* dst = reinterpret_cast<f32x4*>(out + i * 16);
#pragma unroll
  for (int q = 0; q < 4; ++q) dst[q] = f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
}

}  // namespace

extern "C" int dsm_stage_images_nhwc16(const void* left, const void* right, void* out, int B, int C,
                                       int H, int W, dsm_stream_t stream) {
  DSM_REQUIRE(left && out && B > 0 && C > 0 && H > 0 && W > 0, DSM_ERR_ARG);
  DSM_REQUIRE(C <= 16, DSM_ERR_UNSUPPORTED);
  DSM_REQUIRE(dsm_aligned16(out), DSM_ERR_ALIGN);
  const long n = (long)(right ? 2 : 1) * B * H * W;
  DSM_REQUIRE(n / 256 < 0x7fffffffL, DSM_ERR_UNSUPPORTED);
  dsm_clear_stale_error();
  hipLaunchKernelGGL(stage_pair_kernel, dim3(dsm_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const float*)left, (const float*)right, (float*)out, B, C, (long)H * W);
  return dsm_launch_status();
}

extern "C" int dsm_decoder_cat(const void* up, const void* bias, const void* pr, const void* skip,
                               void* out, int B, int Cu, int Cp, int Cs, int Hu, int Wu, int Hp,
                               int Wp, int Hs, int Ws, int relu, dsm_stream_t stream) {
  DSM_REQUIRE(up && out && B > 0 && Cu > 0 && Hu > 0 && Wu > 0, DSM_ERR_ARG);
  DSM_REQUIRE(Cp >= 0 && Cs >= 0 && (Cp == 0 || (pr && Hp > 0 && Wp > 0)) &&
              (Cs == 0 || (skip && Hs > 0 && Ws > 0)), DSM_ERR_ARG);
  DecCatParams p;
  p.up = (const float*)up; p.bias = (const float*)bias; p.pr = (const float*)pr;
  p.skip = (const float*)skip; p.out = (float*)out;
  p.B = B; p.Cu = Cu; p.Cp = Cp; p.Cs = Cs;
  p.Hu = Hu; p.Wu = Wu; p.Hp = Hp; p.Wp = Wp; p.Hs = Hs; p.Ws = Ws;
  p.h = Hu; p.w = Wu;
  if (Cp) { p.h = p.h < 2 * Hp ? p.h : 2 * Hp; p.w = p.w < 2 * Wp ? p.w : 2 * Wp; }
  if (Cs) { p.h = p.h < Hs ? p.h : Hs; p.w = p.w < Ws ? p.w : Ws; }
  p.relu = relu ? 1 : 0;
  const long n = (long)B * (Cu + Cp + Cs) * p.h * ((p.w + 3) / 4);
  DSM_REQUIRE(n / 256 < 0x7fffffffL, DSM_ERR_UNSUPPORTED);
  dsm_clear_stale_error();
  hipLaunchKernelGGL(decoder_cat_kernel, dim3(dsm_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, p);
  return dsm_launch_status();
}

extern "C" int dsm_decoder_cat_bwd(const void* g, const void* out, void* g_up, void* g_bias, void* g_pr,
                                   void* g_skip, int B, int Cu, int Cp, int Cs, int Hu, int Wu, int Hp,
                                   int Wp, int Hs, int Ws, int relu, dsm_stream_t stream) {
  DSM_REQUIRE(g && B > 0 && Cu > 0 && Hu > 0 && Wu > 0, DSM_ERR_ARG);
  DSM_REQUIRE(out || !relu, DSM_ERR_ARG);
  DSM_REQUIRE(Cp >= 0 && Cs >= 0 && (Cp == 0 || (Hp > 0 && Wp > 0)) && (Cs == 0 || (Hs > 0 && Ws > 0)),
              DSM_ERR_ARG);
  DecBwdParams p;
  p.g = (const float*)g; p.out = (const float*)out; p.g_up = (float*)g_up; p.g_bias = (float*)g_bias;
  p.g_pr = (float*)g_pr; p.g_skip = (float*)g_skip;
  p.B = B; p.Cu = Cu; p.Cp = Cp; p.Cs = Cs;
  p.Hu = Hu; p.Wu = Wu; p.Hp = Hp; p.Wp = Wp; p.Hs = Hs; p.Ws = Ws;
  p.h = Hu; p.w = Wu;
  if (Cp) { p.h = p.h < 2 * Hp ? p.h : 2 * Hp; p.w = p.w < 2 * Wp ? p.w : 2 * Wp; }
  if (Cs) { p.h = p.h < Hs ? p.h : Hs; p.w = p.w < Ws ? p.w : Ws; }
  p.relu = relu ? 1 : 0;
  const long per = 256L * DEC_ITER;
  p.cbu = dsm_cdiv((long)Hu * ((Wu + 3) / 4), per);
  p.cbs = Cs ? dsm_cdiv((long)Hs * ((Ws + 3) / 4), per) : 1;
  p.nbu = (g_up || g_bias) ? (long)B * Cu * p.cbu : 0;
  p.nbs = (Cs && g_skip) ? (long)B * Cs * p.cbs : 0;
  const long nbp = (Cp && g_pr) ? ((long)B * Cp * Hp * Wp + 255) / 256 : 0;
  const long nb = p.nbu + p.nbs + nbp;
  DSM_REQUIRE(nb < 0x7fffffffL, DSM_ERR_UNSUPPORTED);
  dsm_clear_stale_error();
  if (g_bias)      // a kernel, not hipMemsetAsync: memset nodes do not replay reliably in a captured graph here
    hipLaunchKernelGGL(decoder_zero_kernel, dim3(dsm_cdiv(Cu, 256)), dim3(256), 0, (hipStream_t)stream,
                       (float*)g_bias, Cu);
  if (nb)
    hipLaunchKernelGGL(decoder_cat_bwd_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, p);
  return dsm_launch_status();
}
