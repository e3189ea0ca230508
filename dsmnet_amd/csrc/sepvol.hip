// First convolution of a concatenation cost volume, from 2-D maps.
//
// Plane d of the volume is [left | right shifted by d] with x < d zeroed, so a 3x3x3 convolution
// over it never needs the volume.  With the column convolutions (dy and channels summed)
//   KL[dz][dx][o, y, s] = sum_{dy,c} W[o, c,     dz, dy, dx] left [c, y + dy, s]
//   KR[dz][dx][o, y, s] = sum_{dy,c} W[o, C + c, dz, dy, dx] right[c, y + dy, s]
// every output element is (dd = d + dz, xx = x + dx, u = x - d)
//   conv[o, d, y, x] = sum over (dz, dx) with 0 <= dd < D, 0 <= xx < W of
//        [xx >= dd or not mask_left] KL[dz][dx][o, y, xx] + [xx >= dd] KR[dz][dx][o, y, xx - dd]
// Away from the x borders and the masked band this is F_v[y, x] + G_v[y, u]: two 2-D images per
// "plane variant" v (which dz exist: all / no -1 (d = 0) / no +1 (d = D-1) / only 0 (D = 1)).
//
//   sepvol_kmaps_kernel      the 18 K images, exact fp32-input MFMA (32 pixels x 32 outputs x 3C)
//   sepvol_sums_kernel       F_v, G_v from the K images
//   sepvol_broadcast_kernel  the (B, D, H, W, 32) output: F + G from LDS (general form from the K
//                            images where it does not apply), folded BN, ReLU, max |y|
#include "split_core.hpp"    // track_amax, publish_amax

namespace {

constexpr int SV_CO = 32;        // output channels
constexpr int SV_NV = 4;         // plane variants

__host__ __device__ inline int sv_variant(int d, int D) { return (d == 0 ? 1 : 0) | (d == D - 1 ? 2 : 0); }
// (variant v keeps dz = -1 unless bit 0, dz = +1 unless bit 1)

// ---------------------------------------------------------------------------------------------
// phase 1a: K[n][dz][dx][y][x][o] for the 2B maps (left maps use W[:, :C], right maps W[:, C:]).
// One wave = 32 pixels of one row; k runs over (dy, c): lane half h holds channels [hC/2, (h+1)C/2).
// wp: [side][dz][dx][dy][cc][h][o] (costvolume.pack_concat_conv_weight).
// ---------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void sepvol_kmaps_kernel(const float* __restrict__ both,
                                                           const float* __restrict__ wp,
                                                           float* __restrict__ kmaps, int B, int H, int W) {
  constexpr int STEPS = 3 * C / 2;              // MFMA k-steps per (dz, dx)
  constexpr int NPRE = STEPS * 64 / 4 / 256;    // f32x4 per thread per (dz, dx) weight slab
  __shared__ float wl[STEPS * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tpr = (W + 31) >> 5;                // 32-pixel tiles per row
  const int n = blockIdx.y, side = n >= B ? 1 : 0;
  const int tile = blockIdx.x * 4 + wave;
  const bool live = tile < H * tpr;
  const int y = live ? tile / tpr : 0, x0 = live ? (tile % tpr) * 32 : 0;
  const int p = lane & 31, h = lane >> 5;

  float a[STEPS];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy) {
    const int yy = y + dy - 1;
    const bool ok = live && yy >= 0 && yy < H && x0 + p < W;
    const f32x4* src = reinterpret_cast<const f32x4*>(both + (((long)n * H + (ok ? yy : 0)) * W + (ok ? x0 + p : 0)) * C + h * (C / 2));
#pragma unroll
    for (int q = 0; q < C / 8; ++q) {
      f32x4 v = ok ? src[q] : f32x4{0.f, 0.f, 0.f, 0.f};
      a[dy * (C / 2) + 4 * q + 0] = v.x; a[dy * (C / 2) + 4 * q + 1] = v.y;
      a[dy * (C / 2) + 4 * q + 2] = v.z; a[dy * (C / 2) + 4 * q + 3] = v.w;
    }
  }

  const f32x4* wsrc = reinterpret_cast<const f32x4*>(wp + (long)side * 9 * STEPS * 64);
  f32x4 pre[NPRE];
#pragma unroll
  for (int i = 0; i < NPRE; ++i) pre[i] = wsrc[i * 256 + threadIdx.x];
  for (int cb = 0; cb < 9; ++cb) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NPRE; ++i) reinterpret_cast<f32x4*>(wl)[i * 256 + threadIdx.x] = pre[i];
    __syncthreads();
    if (cb + 1 < 9) {
#pragma unroll
      for (int i = 0; i < NPRE; ++i) pre[i] = wsrc[(long)(cb + 1) * (STEPS * 16) + i * 256 + threadIdx.x];
    }
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < STEPS; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], wl[j * 64 + lane], acc, 0, 0, 0);
    if (live) {
      float* dst = kmaps + ((((long)n * 9 + cb) * H + y) * W + x0) * SV_CO + p;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
        if (x0 + row < W) dst[(long)row * SV_CO] = acc[r];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// phase 1b: F[b][v][y][x][o] (x in [0, W)) and G[b][v][y][u + 2][o] (u in [-2, W)).
//   F_v[y, x] = sum_{dz in v, dx: 0 <= x + dx < W} KL[dz][dx][y, x + dx]
//   G_v[y, u] = sum_{dz in v, dx: 0 <= u + dx - dz < W} KR[dz][dx][y, u + dx - dz]
// One thread = four channels of one (b, y, column); column c is x = c for F and u = c - 2 for G.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sepvol_sums_kernel(const float* __restrict__ kmaps, float* __restrict__ fmap,
                                                          float* __restrict__ gmap, int B, int H, int W) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const int o4 = (int)(t & 7);
  const long pix = t >> 3;
  const int WG = W + 2;
  if (pix >= (long)B * H * WG) return;
  const int c = (int)(pix % WG), y = (int)((pix / WG) % H), b = (int)(pix / ((long)WG * H));
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 fs[3], gs[3];
#pragma unroll
  for (int z = 0; z < 3; ++z) {
    fs[z] = zero; gs[z] = zero;
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int cb = z * 3 + dx + 1;
      const int xl = c + dx;                            // left: x + dx
      if (c < W && xl >= 0 && xl < W)
        fs[z] += *reinterpret_cast<const f32x4*>(kmaps + ((((long)b * 9 + cb) * H + y) * W + xl) * SV_CO + o4 * 4);
      const int xr = c - 2 + dx - (z - 1);              // right: u + dx - dz
      if (xr >= 0 && xr < W)
        gs[z] += *reinterpret_cast<const f32x4*>(kmaps + ((((long)(B + b) * 9 + cb) * H + y) * W + xr) * SV_CO + o4 * 4);
    }
  }
#pragma unroll
  for (int v = 0; v < SV_NV; ++v) {
    f32x4 f = fs[1], g = gs[1];
    if (!(v & 1)) { f += fs[0]; g += gs[0]; }
    if (!(v & 2)) { f += fs[2]; g += gs[2]; }
    if (c < W) *reinterpret_cast<f32x4*>(fmap + ((((long)b * SV_NV + v) * H + y) * W + c) * SV_CO + o4 * 4) = f;
    *reinterpret_cast<f32x4*>(gmap + ((((long)b * SV_NV + v) * H + y) * WG + c) * SV_CO + o4 * 4) = g;
  }
}

// ---------------------------------------------------------------------------------------------
// phase 2: one workgroup = (b, y, TX columns from x0, PD planes from d0).  LDS: TX pixels of F_v and
// TX + PD - 1 pixels of G_v (u from x0 - (d0 + PD - 1)), refilled when the plane variant changes.
// ---------------------------------------------------------------------------------------------
struct SvBroadcast {
  const float* kmaps; const float* fmap; const float* gmap;
  const float* scale; const float* shift;
  float* y; float* y_amax;
  int B, D, H, W, mask_left, relu, TX, PD, plain_stores;
};

__device__ __forceinline__ f32x4 sv_general(const SvBroadcast& p, int b, int d, int y, int x, int o4) {
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  for (int dz = -1; dz <= 1; ++dz) {
    const int dd = d + dz;
    if (dd < 0 || dd >= p.D) continue;
    for (int dx = -1; dx <= 1; ++dx) {
      const int xx = x + dx;
      if (xx < 0 || xx >= p.W) continue;
      const int cb = (dz + 1) * 3 + dx + 1;
      if (xx >= dd || !p.mask_left)
        s += *reinterpret_cast<const f32x4*>(p.kmaps + ((((long)b * 9 + cb) * p.H + y) * p.W + xx) * SV_CO + o4 * 4);
      if (xx >= dd)
        s += *reinterpret_cast<const f32x4*>(p.kmaps + ((((long)(p.B + b) * 9 + cb) * p.H + y) * p.W + xx - dd) * SV_CO + o4 * 4);
    }
  }
  return s;
}

__global__ __launch_bounds__(256) void sepvol_broadcast_kernel(SvBroadcast p) {
  extern __shared__ __align__(16) float lds[];
  __shared__ float red[4];
  const int TX = p.TX, PD = p.PD, W = p.W, D = p.D, H = p.H;
  const int x0 = blockIdx.x * TX, d0 = blockIdx.y * PD;
  const int y = blockIdx.z % H, b = blockIdx.z / H;
  const int nx = min(TX, W - x0), d1 = min(d0 + PD, D);
  const int ubase = x0 - (d0 + PD - 1);
  const int ng = TX + PD - 1;
  f32x4* fl = reinterpret_cast<f32x4*>(lds);
  f32x4* gl = fl + TX * 8;
  const int o4 = threadIdx.x & 7;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = zero;
  if (p.scale) sc = *reinterpret_cast<const f32x4*>(p.scale + o4 * 4);
  if (p.shift) sh = *reinterpret_cast<const f32x4*>(p.shift + o4 * 4);
  float am = 0.f;
  int cur = -1;
  for (int d = d0; d < d1; ++d) {
    const int v = sv_variant(d, D);
    if (v != cur) {                                    // uniform
      __syncthreads();
      const f32x4* fsrc = reinterpret_cast<const f32x4*>(p.fmap + ((((long)b * SV_NV + v) * H + y) * W + x0) * SV_CO);
      for (int i = threadIdx.x; i < nx * 8; i += 256) fl[i] = fsrc[i];
      const f32x4* gsrc = reinterpret_cast<const f32x4*>(p.gmap + (((long)b * SV_NV + v) * H + y) * (long)(W + 2) * SV_CO);
      for (int i = threadIdx.x; i < ng * 8; i += 256) {
        const int u = ubase + (i >> 3);
        gl[i] = (u >= -2 && u < W) ? gsrc[(u + 2) * 8 + (i & 7)] : zero;
      }
      __syncthreads();
      cur = v;
    }
    f32x4* dst = reinterpret_cast<f32x4*>(p.y + ((((long)b * D + d) * H + y) * W + x0) * SV_CO);
    for (int i = threadIdx.x; i < nx * 8; i += 256) {
      const int xi = i >> 3, x = x0 + xi, u = x - d;
      f32x4 s;
      if (x >= 1 && x <= W - 2 && (!p.mask_left || u >= 2)) s = fl[i] + gl[(u - ubase) * 8 + o4];
      else if (p.mask_left && u <= -3) s = zero;
      else s = sv_general(p, b, d, y, x, o4);
      s = s * sc + sh;
      if (p.relu) { s.x = fmaxf(s.x, 0.f); s.y = fmaxf(s.y, 0.f); s.z = fmaxf(s.z, 0.f); s.w = fmaxf(s.w, 0.f); }
      track_amax(am, s);
      if (p.plain_stores) dst[i] = s; else __builtin_nontemporal_store(s, dst + i);
    }
  }
  publish_amax<4, false>(p.y_amax, am, red);           // `red` is the publisher's own: no barrier ahead of the write
}

}  // namespace

extern "C" int dsm_concat_conv_fwd(const void* both, const void* w_packed, const void* scale, const void* shift,
                                   void* workspace, size_t workspace_floats, void* y, float* y_amax,
                                   int B, int C, int Cout, int D, int H, int W,
                                   int mask_left, int relu, int flags, dsm_stream_t stream) {
  DSM_REQUIRE(both && w_packed && workspace && y, DSM_ERR_ARG);
  DSM_REQUIRE(B >= 1 && C >= 1 && D >= 1 && H >= 1 && W >= 1 && flags >= 0, DSM_ERR_ARG);
  DSM_REQUIRE(C % 32 == 0 && Cout == SV_CO, DSM_ERR_ARG);
  DSM_REQUIRE(C == 32 || C == 64, DSM_ERR_UNSUPPORTED);
  const size_t kfl = (size_t)2 * B * 9 * H * W * SV_CO, ffl = (size_t)B * SV_NV * H * W * SV_CO;
  const size_t gfl = (size_t)B * SV_NV * H * (W + 2) * SV_CO;
  DSM_REQUIRE(workspace_floats >= kfl + ffl + gfl, DSM_ERR_ARG);
  DSM_REQUIRE(dsm_aligned16(both) && dsm_aligned16(w_packed) && dsm_aligned16(workspace) && dsm_aligned16(y) &&
              dsm_aligned16(scale) && dsm_aligned16(shift), DSM_ERR_ALIGN);
  int PD = flags & 0xff, TX = (flags >> 8) & 0xfff;
  if (PD == 0) PD = 12;
  if (TX == 0) TX = 107;
  PD = PD > D ? D : PD;
  TX = TX > W ? W : TX;
  DSM_REQUIRE((size_t)(2 * TX + PD - 1) * SV_CO * 4 <= 64 * 1024, DSM_ERR_ARG);
  DSM_REQUIRE(dsm_cdiv(D, PD) <= 65535 && (long)B * H <= 65535, DSM_ERR_UNSUPPORTED);
  hipStream_t s = (hipStream_t)stream;
  float* kmaps = (float*)workspace;
  float* fmap = kmaps + kfl;
  float* gmap = fmap + ffl;
  dsm_clear_stale_error();
  const int tpr = (W + 31) / 32;
  const dim3 kgrid((unsigned)dsm_cdiv((long)H * tpr, 4), (unsigned)(2 * B));
  if (C == 32)
    hipLaunchKernelGGL(sepvol_kmaps_kernel<32>, kgrid, dim3(256), 0, s, (const float*)both, (const float*)w_packed, kmaps, B, H, W);
  else
    hipLaunchKernelGGL(sepvol_kmaps_kernel<64>, kgrid, dim3(256), 0, s, (const float*)both, (const float*)w_packed, kmaps, B, H, W);
  hipLaunchKernelGGL(sepvol_sums_kernel, dim3((unsigned)dsm_cdiv((long)B * H * (W + 2) * 8, 256)), dim3(256), 0, s,
                     (const float*)kmaps, fmap, gmap, B, H, W);
  SvBroadcast p;
  p.kmaps = kmaps; p.fmap = fmap; p.gmap = gmap;
  p.scale = (const float*)scale; p.shift = (const float*)shift;
  p.y = (float*)y; p.y_amax = y_amax;
  p.B = B; p.D = D; p.H = H; p.W = W; p.mask_left = mask_left ? 1 : 0; p.relu = relu ? 1 : 0; p.TX = TX; p.PD = PD;
  p.plain_stores = (flags >> 20) & 1;
  const dim3 bgrid((unsigned)dsm_cdiv(W, TX), (unsigned)dsm_cdiv(D, PD), (unsigned)(B * H));
  hipLaunchKernelGGL(sepvol_broadcast_kernel, bgrid,
                     dim3(256), (size_t)(2 * TX + PD - 1) * SV_CO * 4, s, p);
  return dsm_launch_status();
}
