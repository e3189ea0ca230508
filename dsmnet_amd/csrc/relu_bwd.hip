// Backward of bias + ReLU behind the wide 2-D layers (conv_wide2d.hpp; costvolume.WideConv2dReLUFunction):
//   g[m][c] = y[m][c] > 0 ? gy[m][c] : 0,   db[c] = sum_m g[m][c],   *g_amax = max(*g_amax, max |g|)
// on NHWC tensors viewed as [M][C], C % 4 == 0.  In the reference this is autograd through nn.ReLU and the
// bias of nn.Conv2d (models/util_conv.py conv2d_bn with bn = False).
//
// One memory-bound pass of 12 B per element (two 16-byte loads, one 16-byte store per lane), then a tiny
// second launch for the bias gradient.  The sum runs in a FIXED order, without float atomics:
//  * workgroup w of G = min(512, ceil(M / 8)) owns the rows [w M / G, (w + 1) M / G);
//  * inside it a thread owns one channel quad and every RL-th row (RL = 256 / min(C / 4, 256) row lanes),
//    adds them in row order, and the row lanes meet in LDS, added in lane order;
//  * the G partial sums go to ws[w][C] with plain stores and the second launch adds them in index order.
// Two runs give the same bits.  ws: G * C floats -- 512 * C always suffices; not read when db is NULL.
#include "conv_common.hpp"

namespace {

constexpr int RB_THREADS = 256, RB_MAX_GROUPS = 512;

__global__ __launch_bounds__(RB_THREADS) void bias_relu_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ y,
                                                                   float* __restrict__ g, float* __restrict__ ws,
                                                                   float* g_amax, long M, int C) {
  __shared__ f32x4 part[RB_THREADS];
  __shared__ float red[4];
  const int CQ = C >> 2;
  const int CT = CQ < RB_THREADS ? CQ : RB_THREADS;    // channel quads side by side
  const int RL = RB_THREADS / CT;                      // row lanes (1 when C >= 1024)
  const int tid = threadIdx.x, rl = tid / CT, ct = tid % CT;
  const long r0 = (long)blockIdx.x * M / gridDim.x, r1 = (long)(blockIdx.x + 1) * M / gridDim.x;
  float am = 0.f;
  for (int cb = 0; cb < CQ; cb += CT) {                // uniform trip count (barriers inside)
    const int cq = cb + ct;
    const bool on = rl < RL && cq < CQ;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (on) {
#pragma unroll 4
      for (long m = r0 + rl; m < r1; m += RL) {
        const long e = m * CQ + cq;
        const f32x4 a = reinterpret_cast<const f32x4*>(gy)[e];
        const f32x4 b = reinterpret_cast<const f32x4*>(y)[e];
        f32x4 v;
        v.x = b.x > 0.f ? a.x : 0.f; v.y = b.y > 0.f ? a.y : 0.f;
        v.z = b.z > 0.f ? a.z : 0.f; v.w = b.w > 0.f ? a.w : 0.f;
        reinterpret_cast<f32x4*>(g)[e] = v;
        acc += v;
        track_amax(am, v);
      }
    }
    if (ws) {                                          // uniform
      __syncthreads();                                 // the previous column tile's sums have been read
      part[tid] = acc;
      __syncthreads();
      if (rl == 0 && cq < CQ) {
        f32x4 s = part[ct];
        for (int k = 1; k < RL; ++k) s += part[k * CT + ct];
        reinterpret_cast<f32x4*>(ws)[(long)blockIdx.x * CQ + cq] = s;
      }
    }
  }
  publish_amax<4>(g_amax, am, red);
}

// db[c] = the workgroups' partial sums, added in index order
__global__ __launch_bounds__(64) void bias_relu_bwd_sum_kernel(const float* __restrict__ ws, float* __restrict__ db,
                                                               int G, int C) {
  const int CQ = C >> 2, cq = blockIdx.x * 64 + threadIdx.x;
  if (cq >= CQ) return;
  f32x4 s = reinterpret_cast<const f32x4*>(ws)[cq];
  for (int k = 1; k < G; ++k) s += reinterpret_cast<const f32x4*>(ws)[(long)k * CQ + cq];
  reinterpret_cast<f32x4*>(db)[cq] = s;
}

}  // namespace

extern "C" int dsm_bias_relu_bwd(const void* gy, const void* y, void* g, void* db, void* ws, float* g_amax,
                                 long M, int C, dsm_stream_t stream) {
  DSM_REQUIRE(gy && y && g && g != gy && g != y, DSM_ERR_ARG);
  DSM_REQUIRE(M > 0 && C > 0 && (!db || ws), DSM_ERR_ARG);
  DSM_REQUIRE(C % 4 == 0 && M < (1l << 40) / C, DSM_ERR_UNSUPPORTED);
  DSM_REQUIRE(dsm_aligned16(gy) && dsm_aligned16(y) && dsm_aligned16(g) && dsm_aligned16(db) &&
              (!db || dsm_aligned16(ws)), DSM_ERR_ALIGN);
  const long want = (M + 7) / 8;
  const int G = (int)(want < RB_MAX_GROUPS ? want : RB_MAX_GROUPS);
  hipStream_t s = (hipStream_t)stream;
  dsm_clear_stale_error();
  hipLaunchKernelGGL(bias_relu_bwd_kernel, dim3(G), dim3(RB_THREADS), 0, s, (const float*)gy, (const float*)y,
                     (float*)g, db ? (float*)ws : nullptr, g_amax, M, C);
  if (db)
    hipLaunchKernelGGL(bias_relu_bwd_sum_kernel, dim3(dsm_cdiv(C / 4, 64)), dim3(64), 0, s, (const float*)ws,
                       (float*)db, G, C);
  return dsm_launch_status();
}
