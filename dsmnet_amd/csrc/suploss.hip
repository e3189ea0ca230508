// Supervised pyramid loss and the D1 / EPE metrics (losses/loss.py:326-338 loss_supervised,
// :36-44 diff1_dx / diff1_dy, :407-421 losses_pyramid0; stereo.py:103-113 accuracy), fused.
//
// Stock torch runs, per weighted output and in both directions, a bilinear upsampling by
// 2^level, a crop, sub / abs / a boolean gather / mean, two padded first differences, abs / add /
// clamp / a second gather / a second mean -- with a host read for "any valid pixel" and one per
// boolean index.  Here the whole pyramid (every weighted output) is ONE work list of 16x64
// fine-resolution tiles:
//   forward   suploss_fwd_tiles   per (tile, item): the coarse patch under the tile and its
//                                 one-pixel halo staged in LDS, the bilinear samples p of the
//                                 tile + halo formed there once, then per pixel m = gt > 0,
//                                 |gt - p|, dx / dy (zero in the last column / row of the
//                                 CROPPED image), min(|dx| + |dy|, 1), the "good pixel" test of
//                                 accuracy; per-tile partial sums {sum m|gt-p|, sum m*sm, n, good}
//                                 to a slab with plain stores; when a gradient is wanted, the
//                                 unnormalised fine-pixel gradient (4 B per pixel per item)
//             suploss_reduce      one workgroup: the slabs summed in a fixed order (fp64), the
//                                 loss and aux = n, then per item L1 mean, smooth mean, EPE, D1 %
//   backward  suploss_bwd_gather  a GATHER: one coarse element sums, in fp64 and in a fixed order,
//                                 the saved fine gradients whose bilinear taps touch it (2^level
//                                 wide lane groups, up to a whole wave per element), scaled by
//                                 grad_loss * weight / n read on the device.  No atomics anywhere.
//
// The upsampling is F.interpolate(scale_factor = 2^level, mode="bilinear", align_corners=False)
// as this torch computes it: source coordinate max((X + 0.5) / s - 0.5, 0), second tap clamped
// at the last index.  The smoothness adjoint passes where |dx| + |dy| <= 1 (torch.clamp's
// inclusive rule) with sign(0) = 0 (torch.abs).  No valid pixel: loss 0, gradients 0.
#include "common.hpp"

namespace {

constexpr int TH = 16, TW = 64;            // fine tile: 1024 pixels, four per thread
constexpr int PH = TH + 2, PW = TW + 2;    // prediction region: one-pixel halo on every side
constexpr int GH = TH + 1, GW = TW + 1;    // ground-truth region: halo above and to the left
constexpr int NPART = 4;                   // partial sums per (tile, item)
constexpr int MAX_LEVEL = 12;
static_assert(sizeof(dsm_suploss_item) == 48, "dsm_suploss_item layout (ctypes mirror in _lib.py)");

struct Work {
  dsm_suploss_item it[DSM_SUPLOSS_MAX_ITEMS];
  int bwd0[DSM_SUPLOSS_MAX_ITEMS + 1];     // first backward workgroup of each item
  int n, B, H, W, nty, ntx, per;           // per = tiles of one item = B * nty * ntx
  int flag_smooth, save, vec_gt;
  unsigned vec_pred;                       // bit i: item i's map takes 16-byte accesses
  const float* gt;
  float* part;                             // [item][tile][NPART]
  float* saved;                            // [item][B*H*W]
};

// one axis of upsample_bilinear2d (align_corners = False, scale_factor given)
struct Tap {
  int i0, i1;
  float l0, l1;
};

__device__ __forceinline__ Tap tap_at(int dst, float inv, int size) {
  Tap t;
  const float src = fmaxf(inv * ((float)dst + 0.5f) - 0.5f, 0.f);
  t.i0 = min((int)src, size - 1);
  t.i1 = t.i0 + (t.i0 < size - 1 ? 1 : 0);
  t.l1 = fminf(fmaxf(src - (float)t.i0, 0.f), 1.f);
  t.l0 = 1.f - t.l1;
  return t;
}

__device__ __forceinline__ float tap_weight(const Tap& t, int c) {
  return (t.i0 == c ? t.l0 : 0.f) + (t.i1 == c ? t.l1 : 0.f);
}

__device__ __forceinline__ int sgni(float v) { return (v > 0.f) - (v < 0.f); }

__global__ __launch_bounds__(256) void suploss_fwd_tiles(const Work K) {
  __shared__ float C[PH * PW];             // coarse patch (levels > 0)
  __shared__ float P[PH][PW];              // fine prediction, rows ty0-1.., columns tx0-1..
  __shared__ float G[GH][GW];              // ground truth, rows ty0-1.., columns tx0-1..
  __shared__ float red[4][NPART];
  const int tid = threadIdx.x;
  const int i = blockIdx.x / K.per;
  int local = blockIdx.x - i * K.per;
  const int b = local / (K.nty * K.ntx);
  local -= b * (K.nty * K.ntx);
  const int ty0 = (local / K.ntx) * TH, tx0 = (local % K.ntx) * TW;
  const dsm_suploss_item& it = K.it[i];
  const int H = K.H, W = K.W, hc = it.hc, wc = it.wc;
  const float* pred = (const float*)it.pred + (long)b * hc * wc;
  const float* gt = K.gt + (long)b * H * W;

  // 1. ground truth: one 16-byte load per thread, the halo row and column with scalar loads
  {
    const int r = tid / (TW / 4), c4 = (tid % (TW / 4)) * 4;
    const int y = ty0 + r, x = tx0 + c4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (y < H) {
      const float* row = gt + (long)y * W;
      if (K.vec_gt && x < W) {             // W % 4 == 0: the four pixels are inside together
        const f32x4 q = *(const f32x4*)(row + x);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (x + k < W) v[k] = row[x + k];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) G[r + 1][c4 + 1 + k] = v[k];
    if (tid < GW) {
      const int yy = ty0 - 1, xx = tx0 - 1 + tid;
      G[0][tid] = (yy >= 0 && xx >= 0 && xx < W) ? gt[(long)yy * W + xx] : 0.f;
    } else if (tid < GW + TH) {
      const int rr = tid - GW, yy = ty0 + rr, xx = tx0 - 1;
      G[rr + 1][0] = (xx >= 0 && yy < H) ? gt[(long)yy * W + xx] : 0.f;
    }
  }

  // 2. the prediction at fine resolution over the tile and its halo
  if (it.level == 0) {
    const bool vec = (K.vec_pred >> i) & 1u;
    for (int v = tid; v < PH * (TW / 4); v += 256) {
      const int r = v / (TW / 4), c4 = (v % (TW / 4)) * 4;
      const int y = ty0 - 1 + r, x = tx0 + c4;
      float q[4] = {0.f, 0.f, 0.f, 0.f};
      if (y >= 0 && y < hc) {
        const float* row = pred + (long)y * wc;
        if (vec && x < wc) {
          const f32x4 t = *(const f32x4*)(row + x);
          q[0] = t.x; q[1] = t.y; q[2] = t.z; q[3] = t.w;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (x + k < wc) q[k] = row[x + k];
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) P[r][c4 + 1 + k] = q[k];
    }
    for (int v = tid; v < 2 * PH; v += 256) {
      const int r = v >> 1, side = v & 1;
      const int y = ty0 - 1 + r, x = side ? tx0 + TW : tx0 - 1;
      P[r][side ? PW - 1 : 0] = (y >= 0 && y < hc && x >= 0 && x < wc) ? pred[(long)y * wc + x] : 0.f;
    }
  } else {
    const float inv = 1.f / (float)(1 << it.level);
    const int Y0 = max(ty0 - 1, 0), Y1 = min(ty0 + TH, H - 1);
    const int X0 = max(tx0 - 1, 0), X1 = min(tx0 + TW, W - 1);
    const int cy0 = tap_at(Y0, inv, hc).i0, cx0 = tap_at(X0, inv, wc).i0;
    const int ph = tap_at(Y1, inv, hc).i1 - cy0 + 1, pw = tap_at(X1, inv, wc).i1 - cx0 + 1;
    for (int v = tid; v < ph * pw; v += 256)       // at most 11 x 35 elements: s >= 2
      C[v] = pred[(long)(cy0 + v / pw) * wc + cx0 + v % pw];
    __syncthreads();
    for (int v = tid; v < PH * PW; v += 256) {
      const int r = v / PW, c = v % PW;
      const int Y = ty0 - 1 + r, X = tx0 - 1 + c;
      float val = 0.f;
      if (Y >= 0 && Y < H && X >= 0 && X < W) {
        const Tap ty = tap_at(Y, inv, hc), tx = tap_at(X, inv, wc);
        const float* r0 = C + (ty.i0 - cy0) * pw - cx0;
        const float* r1 = C + (ty.i1 - cy0) * pw - cx0;
        val = ty.l0 * (tx.l0 * r0[tx.i0] + tx.l1 * r0[tx.i1]) +
              ty.l1 * (tx.l0 * r1[tx.i0] + tx.l1 * r1[tx.i1]);
      }
      P[r][c] = val;
    }
  }
  __syncthreads();

  // 3. the pixel terms: consecutive lanes take consecutive columns
  float part[NPART] = {0.f, 0.f, 0.f, 0.f};
  float* sv = K.save ? K.saved + ((long)i * K.B + b) * H * W : nullptr;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int idx = k * 256 + tid;
    const int r = idx / TW, c = idx % TW;
    const int y = ty0 + r, x = tx0 + c;
    if (y >= H || x >= W) continue;
    const float g = G[r + 1][c + 1], p = P[r + 1][c + 1];
    const bool m = g > 0.f;
    const float e = fabsf(g - p);
    const float dx = x + 1 < W ? P[r + 1][c + 2] - p : 0.f;
    const float dy = y + 1 < H ? P[r + 2][c + 1] - p : 0.f;
    const float mag = fabsf(dx) + fabsf(dy);
    if (m) {
      part[0] += e;
      part[1] += fminf(mag, 1.f);
      part[2] += 1.f;
      part[3] += (e <= 3.f || e / g <= 0.05f) ? 1.f : 0.f;
    }
    if (sv) {
      // d/dp of m|gt - p| + 0.1 (m sm): the pixel's own -dx / -dy terms and the +dx / +dy
      // terms of its left / upper neighbour, each under that pixel's mask and clamp
      int s0 = m ? sgni(p - g) : 0, ks = 0;
      if (K.flag_smooth) {
        if (m && mag <= 1.f) ks -= sgni(dx) + sgni(dy);
        if (x > 0 && G[r + 1][c] > 0.f) {
          const float pl = P[r + 1][c];
          const float dxl = p - pl, dyl = y + 1 < H ? P[r + 2][c] - pl : 0.f;
          if (fabsf(dxl) + fabsf(dyl) <= 1.f) ks += sgni(dxl);
        }
        if (y > 0 && G[r][c + 1] > 0.f) {
          const float pu = P[r][c + 1];
          const float dyu = p - pu, dxu = x + 1 < W ? P[r][c + 2] - pu : 0.f;
          if (fabsf(dxu) + fabsf(dyu) <= 1.f) ks += sgni(dyu);
        }
      }
      sv[(long)y * W + x] = (float)s0 + 0.1f * (float)ks;
    }
  }
  const int wave = tid / 64, lane = tid % 64;
#pragma unroll
  for (int k = 0; k < NPART; ++k) {
    const float s = wave_sum(part[k]);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  if (tid < NPART)
    K.part[(long)blockIdx.x * NPART + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// one workgroup; every sum in a fixed order (fp64), so the loss is bit-reproducible
__global__ __launch_bounds__(256) void suploss_reduce(const Work K, float* loss, float* aux) {
  __shared__ double red[NPART][256];
  __shared__ double sums[DSM_SUPLOSS_MAX_ITEMS][NPART];
  const int tid = threadIdx.x;
  for (int i = 0; i < K.n; ++i) {
    double s[NPART] = {0.0, 0.0, 0.0, 0.0};
    const float* slab = K.part + (long)i * K.per * NPART;
    for (int t = tid; t < K.per; t += 256) {
      const f32x4 q = *(const f32x4*)(slab + (long)t * NPART);
      s[0] += (double)q.x; s[1] += (double)q.y; s[2] += (double)q.z; s[3] += (double)q.w;
    }
#pragma unroll
    for (int k = 0; k < NPART; ++k) red[k][tid] = s[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) {
#pragma unroll
        for (int k = 0; k < NPART; ++k) red[k][tid] += red[k][tid + o];
      }
      __syncthreads();
    }
    if (tid < NPART) sums[i][tid] = red[tid][0];
    __syncthreads();
  }
  if (tid != 0) return;
  const double n = sums[0][2];             // the mask is the ground truth's: the same for every item
  const float nan = __builtin_nanf("");
  double total = 0.0;
  for (int i = 0; i < K.n; ++i) {
    const double l1 = n > 0.0 ? sums[i][0] / n : 0.0;
    const double sm = n > 0.0 ? sums[i][1] / n : 0.0;
    total += (double)K.it[i].weight * (l1 + (K.flag_smooth ? 0.1 * sm : 0.0));
    aux[1 + 4 * i + 0] = (float)l1;
    aux[1 + 4 * i + 1] = (float)sm;
    // accuracy() divides by the pixel count: NaN without ground truth, as there
    aux[1 + 4 * i + 2] = n > 0.0 ? (float)l1 : nan;
    aux[1 + 4 * i + 3] = n > 0.0 ? (float)(100.0 - 100.0 * sums[i][3] / n) : nan;
  }
  aux[0] = (float)n;
  loss[0] = (float)total;
}

__device__ __forceinline__ int find_bwd_item(const Work& K, int blk) {
  int i = 0;
  while (i + 1 < K.n && blk >= K.bwd0[i + 1]) ++i;
  return i;
}

// lanes per coarse element: the footprint is 2s fine columns wide (one at level 0)
__host__ __device__ __forceinline__ int group_lanes(int level) {
  return level == 0 ? 1 : (level >= 5 ? 64 : 2 << level);
}

__global__ __launch_bounds__(256) void suploss_bwd_gather(const Work K, const float* __restrict__ aux,
                                                          const float* __restrict__ gloss) {
  const int tid = threadIdx.x;
  const int i = find_bwd_item(K, blockIdx.x);
  const dsm_suploss_item& it = K.it[i];
  const int blk = blockIdx.x - K.bwd0[i];
  const int H = K.H, W = K.W, hc = it.hc, wc = it.wc;
  const long nel = (long)K.B * hc * wc;
  const float n = aux[0];
  const double sc = n > 0.f ? (double)gloss[0] * (double)it.weight / (double)n : 0.0;
  const float* u = K.saved + (long)i * K.B * H * W;
  float* grad = (float*)it.grad;

  if (it.level == 0) {
    if ((K.vec_pred >> i) & 1u && hc == H && wc == W) {       // same grid: 16 bytes per lane
      const long e = ((long)blk * 256 + tid) * 4;
      if (e < nel) {
        const f32x4 q = *(const f32x4*)(u + e);
        f32x4 o;
        o.x = (float)(sc * (double)q.x); o.y = (float)(sc * (double)q.y);
        o.z = (float)(sc * (double)q.z); o.w = (float)(sc * (double)q.w);
        *(f32x4*)(grad + e) = o;
      }
      return;
    }
    const long e = (long)blk * 256 + tid;
    if (e >= nel) return;
    const int cx = (int)(e % wc), cy = (int)((e / wc) % hc), b = (int)(e / ((long)wc * hc));
    const float v = (cy < H && cx < W) ? u[((long)b * H + cy) * W + cx] : 0.f;
    grad[e] = (float)(sc * (double)v);
    return;
  }

  const int s = 1 << it.level, g = group_lanes(it.level);
  const float inv = 1.f / (float)s;
  const int lane = tid % 64;
  const long e = ((long)blk * 4 + tid / 64) * (64 / g) + lane / g;
  const int j = lane % g;
  double acc = 0.0;
  if (e < nel) {
    const int cx = (int)(e % wc), cy = (int)((e / wc) % hc), b = (int)(e / ((long)wc * hc));
    // fine pixels whose taps can touch (cy, cx); tap_weight() is zero for the others, and
    // covers the clamped first / last taps
    const int Ylo = max(0, s * cy - s / 2), Yhi = min(H - 1, s * cy + 3 * s / 2 - 1);
    const int Xlo = max(0, s * cx - s / 2), Xhi = min(W - 1, s * cx + 3 * s / 2 - 1);
    for (int Y = Ylo; Y <= Yhi; ++Y) {
      const float wy = tap_weight(tap_at(Y, inv, hc), cy);
      const float* row = u + ((long)b * H + Y) * W;
      for (int X = Xlo + j; X <= Xhi; X += g) {
        const float wx = tap_weight(tap_at(X, inv, wc), cx);
        acc += (double)row[X] * (double)(wy * wx);
      }
    }
  }
  for (int o = g >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (e < nel && j == 0) grad[e] = (float)(sc * acc);
}

long bwd_blocks(const Work& K, int i) {
  const dsm_suploss_item& it = K.it[i];
  const long nel = (long)K.B * it.hc * it.wc;
  if (it.level == 0) {
    const bool vec = ((K.vec_pred >> i) & 1u) && it.hc == K.H && it.wc == K.W;
    return vec ? (nel / 4 + 255) / 256 : (nel + 255) / 256;
  }
  const long per_block = 4 * (64 / group_lanes(it.level));
  return (nel + per_block - 1) / per_block;
}

int make_work(const dsm_suploss_item* items, int n, const void* gt, int H, int W, int flag_smooth,
              int save, void* workspace, bool backward, Work& K) {
  DSM_REQUIRE(items && gt && workspace, DSM_ERR_ARG);
  DSM_REQUIRE(n >= 1 && n <= DSM_SUPLOSS_MAX_ITEMS, DSM_ERR_ARG);
  DSM_REQUIRE(H > 0 && W > 0, DSM_ERR_ARG);
  const int B = items[0].B;
  for (int i = 0; i < n; ++i) {
    const dsm_suploss_item& it = items[i];
    DSM_REQUIRE(it.pred && it.B > 0 && it.B == B && it.hc > 0 && it.wc > 0 && it.level >= 0, DSM_ERR_ARG);
  }
  DSM_REQUIRE((long)B * H * W < (1L << 31), DSM_ERR_UNSUPPORTED);
  K.n = n; K.B = B; K.H = H; K.W = W;
  K.nty = dsm_cdiv(H, TH); K.ntx = dsm_cdiv(W, TW);
  const long per = (long)B * K.nty * K.ntx;
  DSM_REQUIRE(per * n < (1L << 30), DSM_ERR_UNSUPPORTED);
  K.per = (int)per;
  K.flag_smooth = flag_smooth ? 1 : 0;
  K.save = save ? 1 : 0;
  K.gt = (const float*)gt;
  K.part = (float*)workspace;
  K.saved = K.part + per * n * NPART;
  DSM_REQUIRE(dsm_aligned16(K.part), DSM_ERR_ALIGN);
  K.vec_gt = (W % 4 == 0 && dsm_aligned16(gt)) ? 1 : 0;
  K.vec_pred = 0;
  long blocks = 0;
  for (int i = 0; i < n; ++i) {
    const dsm_suploss_item& it = items[i];
    DSM_REQUIRE(it.level <= MAX_LEVEL, DSM_ERR_UNSUPPORTED);
    DSM_REQUIRE(((long)it.hc << it.level) >= H && ((long)it.wc << it.level) >= W, DSM_ERR_UNSUPPORTED);
    DSM_REQUIRE((long)B * it.hc * it.wc < (1L << 31), DSM_ERR_UNSUPPORTED);
    K.it[i] = it;
    // 16-byte accesses: the map's rows, the saved plane's rows and (backward) the gradient
    if (it.wc % 4 == 0 && dsm_aligned16(it.pred) && (!backward || !it.grad || dsm_aligned16(it.grad)))
      K.vec_pred |= 1u << i;
    K.bwd0[i] = (int)blocks;
    if (backward && it.grad) blocks += bwd_blocks(K, i);
    DSM_REQUIRE(blocks < (1L << 30), DSM_ERR_UNSUPPORTED);
  }
  K.bwd0[n] = (int)blocks;
  return DSM_OK;
}

}  // namespace

extern "C" size_t dsm_suploss_workspace_floats(int n_items, int B, int H, int W, int save_for_bwd) {
  if (n_items < 1 || n_items > DSM_SUPLOSS_MAX_ITEMS || B <= 0 || H <= 0 || W <= 0) return 0;
  const size_t tiles = (size_t)B * dsm_cdiv(H, TH) * dsm_cdiv(W, TW);
  return (size_t)n_items * (tiles * NPART + (save_for_bwd ? (size_t)B * H * W : 0));
}

extern "C" int dsm_suploss_fwd(const dsm_suploss_item* items, int n_items, const void* gt, int H, int W,
                               int flag_smooth, int save_for_bwd, void* workspace, void* loss, void* aux,
                               dsm_stream_t stream) {
  DSM_REQUIRE(loss && aux, DSM_ERR_ARG);
  Work K;
  const int rc = make_work(items, n_items, gt, H, W, flag_smooth, save_for_bwd, workspace, false, K);
  if (rc != DSM_OK) return rc;
  dsm_clear_stale_error();
  hipLaunchKernelGGL(suploss_fwd_tiles, dim3(K.per * K.n), dim3(256), 0, (hipStream_t)stream, K);
  hipLaunchKernelGGL(suploss_reduce, dim3(1), dim3(256), 0, (hipStream_t)stream, K, (float*)loss,
                     (float*)aux);
  return dsm_launch_status();
}

extern "C" int dsm_suploss_bwd(const dsm_suploss_item* items, int n_items, const void* gt, int H, int W,
                               int flag_smooth, const void* workspace, const void* aux,
                               const void* grad_loss, dsm_stream_t stream) {
  DSM_REQUIRE(aux && grad_loss, DSM_ERR_ARG);
  Work K;
  const int rc = make_work(items, n_items, gt, H, W, flag_smooth, 1, (void*)workspace, true, K);
  if (rc != DSM_OK) return rc;
  if (K.bwd0[K.n] == 0) return DSM_OK;     // no item asks for a gradient
  dsm_clear_stale_error();
  hipLaunchKernelGGL(suploss_bwd_gather, dim3(K.bwd0[K.n]), dim3(256), 0, (hipStream_t)stream, K,
                     (const float*)aux, (const float*)grad_loss);
  return dsm_launch_status();
}
