// 1-D left/right feature correlation (DispNetC / iResNet) for gfx950.
//
// Replaces Corr1d.forward, models/util_conv.py:71-86: a python loop that, per
// disparity, materialises a (B,C,H,W-d) product, reduces it over C and slice-assigns
// one plane (~3 launches and ~4*C*H*W*4 bytes per plane).  Here one launch reads
// each feature row once: a workgroup stages fL[b,:,y,x0:x0+64] and the shifted
// window fR[b,:,y,x0-Dpad*s:x0+64] in LDS per 32-channel chunk, and each thread
// owns a 4(x) x 8(d) register block, fed by 16-B LDS reads (1 for fL, 3 or 5 for
// the fR window) -- 32 FMAs per 4 or 6 ds_read_b128, which balances LDS and VALU.
//
// Algorithmic bytes: 2*C*H*W*4 + D*H*W*4; DispNetC 384x1280
// = 36.5 MB, i.e. Infinity-Cache resident and launch/latency scale (about 6 us at
// HBM rate) -- reported as such, not as an HBM fraction.
//
// Corr1d's `simfun` (util_conv.py:57-66): the correlation kernels carry a compile-time SIM; DSM_SIM_COSINE
// (nn.CosineSimilarity(dim=1), each norm clamped at eps on its own) adds a norm pre-pass and an epilogue, and
// in the backward a pre-pass and an epilogue term around the dot-product data gradient, which has an LDS-tiled
// form (corr1d_bwd_tile_kernel) beside the one-thread-per-element one.  Formulas: include/dsmnet_hip.h;
// measurements: profiles/corr1d_sim.md.
#include "common.hpp"

namespace {
constexpr int TX = 64;     // x per workgroup
constexpr int DB = 8;      // disparities per thread
constexpr int CC = 32;     // channels per LDS chunk

__device__ __forceinline__ f32x4 load4_guarded(const float* __restrict__ row, int x, int W,
                                               bool vec) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (vec && x >= 0 && x + 3 < W) return *reinterpret_cast<const f32x4*>(row + x);
  if (x + 0 >= 0 && x + 0 < W) v.x = row[x + 0];
  if (x + 1 >= 0 && x + 1 < W) v.y = row[x + 1];
  if (x + 2 >= 0 && x + 2 < W) v.z = row[x + 2];
  if (x + 3 >= 0 && x + 3 < W) v.w = row[x + 3];
  return v;
}

// Cosine epilogue (SIM = DSM_SIM_COSINE): the sums of columns x .. x+3 of the plane with shift sh = d * S
// times a(x) * r(x - sh); inv = [2][B][H][W] (a of fL, then r of fR), row = (b H + y) W, npix = B H W.
__device__ __forceinline__ void cos_scale4(float (&v)[4], const float* __restrict__ inv, long npix,
                                           long row, int x, int sh, int W) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int xx = x + j, xs = xx - sh;
    if (xx < W) v[j] = xs >= 0 ? v[j] * (inv[row + xx] * inv[npix + row + xs]) : 0.f;
  }
}
}  // namespace

// grid (ceil(W/64), H, B); block = 16 * ceil(D/8) threads rounded up to a wave.
// SIM (all three correlation kernels): DSM_SIM_DOT stores the sums; DSM_SIM_COSINE multiplies them by
// a(x) r(x - d S) from `inv` before the store (cos_scale4) -- the only difference between the two.
template <int S, int SIM>
__global__ __launch_bounds__(256) void corr1d_fwd_kernel(
    const float* __restrict__ fL, const float* __restrict__ fR, float* __restrict__ out,
    const float* __restrict__ inv, int C, int H, int W, int D, int vec) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int ndg = (D + DB - 1) / DB;
  const int padl = ndg * DB * S;            // left halo of the fR window (multiple of 8)
  const int RW = TX + padl;                 // fR columns; column j <-> x = x0 - padl + j
  float* Ls = lds;                          // [CC][TX]
  float* Rs = lds + CC * TX;                // [CC][RW]
  const int x0 = blockIdx.x * TX, y = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int xg = tid & 15, dg = tid >> 4;
  const bool worker = dg < ndg;
  const int d0 = dg * DB;
  constexpr int WIN = 4 + DB * S;           // floats of the fR window per thread
  float acc[DB][4];
#pragma unroll
  for (int i = 0; i < DB; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0.f;

  for (int c0 = 0; c0 < C; c0 += CC) {
    const int cc = min(CC, C - c0);
    __syncthreads();
    for (int i = tid; i < cc * (TX / 4); i += nt) {
      const int c = i / (TX / 4), k = i % (TX / 4);
      const float* row = fL + (((long)b * C + c0 + c) * H + y) * W;
      *reinterpret_cast<f32x4*>(&Ls[c * TX + 4 * k]) = load4_guarded(row, x0 + 4 * k, W, vec);
    }
    const int r4 = RW / 4;
    for (int i = tid; i < cc * r4; i += nt) {
      const int c = i / r4, k = i % r4;
      const float* row = fR + (((long)b * C + c0 + c) * H + y) * W;
      *reinterpret_cast<f32x4*>(&Rs[c * RW + 4 * k]) =
          load4_guarded(row, x0 - padl + 4 * k, W, vec);
    }
    __syncthreads();
    if (worker) {
      const float* lp = Ls + 4 * xg;
      const float* rp = Rs + 4 * xg + padl - (d0 + DB) * S;   // 16-B aligned
      for (int c = 0; c < cc; ++c) {
        const f32x4 l = *reinterpret_cast<const f32x4*>(lp + c * TX);
        float win[WIN];
#pragma unroll
        for (int k = 0; k < WIN / 4; ++k) {
          const f32x4 r = *reinterpret_cast<const f32x4*>(rp + c * RW + 4 * k);
          win[4 * k] = r.x; win[4 * k + 1] = r.y; win[4 * k + 2] = r.z; win[4 * k + 3] = r.w;
        }
#pragma unroll
        for (int i = 0; i < DB; ++i) {
          // output x = x0+4xg+j pairs with fR column (x - (d0+i)S) = window[j + (DB-i)S]
          acc[i][0] = fmaf(l.x, win[0 + (DB - i) * S], acc[i][0]);
          acc[i][1] = fmaf(l.y, win[1 + (DB - i) * S], acc[i][1]);
          acc[i][2] = fmaf(l.z, win[2 + (DB - i) * S], acc[i][2]);
          acc[i][3] = fmaf(l.w, win[3 + (DB - i) * S], acc[i][3]);
        }
      }
    }
  }
  if (!worker) return;
  const int x = x0 + 4 * xg;
  if (x >= W) return;
#pragma unroll
  for (int i = 0; i < DB; ++i) {
    const int d = d0 + i;
    if (d >= D) break;
    float* o = out + (((long)b * D + d) * H + y) * W + x;
    if constexpr (SIM == DSM_SIM_COSINE)
      cos_scale4(acc[i], inv, (long)gridDim.z * H * W, ((long)b * H + y) * W, x, d * S, W);
    if (vec && x + 3 < W) {
      f32x4 v = {acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
      *reinterpret_cast<f32x4*>(o) = v;
    } else {
      for (int j = 0; j < 4 && x + j < W; ++j) o[j] = acc[i][j];
    }
  }
}

// ----------------------------------------------------------------------------
// The tile kernel (r03): stride 1 | 2, W % 4 == 0, D <= 4 DB NDH.
// Workgroup = (b, y, 64 x), 4 NDH waves: wave = (channel quarter cw, d half dh).  What the r01 kernel
// above does in four stage -> barrier -> compute -> barrier rounds with <1 wave per SIMD (40 us for
// 36.5 MB that fit the Infinity Cache) happens here without a barrier before the reduction:
//  * only the fR window [x0 - 4 DB NDH S, x0 + 64) goes through LDS (57 KB at C = 128, D <= 48: two
//    workgroups per CU, the whole 384x1280 problem resident at once); every wave stages the rows of
//    ITS OWN channels -- all its 16-byte loads in flight together, no workgroup barrier -- and reads
//    them back wave-locally;
//  * the fL quad of a lane's four columns comes straight from global memory (the four d-group lanes of
//    a column share the address), a four-deep register ring ahead of its use;
//  * lane = (xg 0..15, dg 0..3) owns a 4(x) x DB(d) register block: per channel (4 + DB S)/4
//    ds_read_b128 feed 4 DB FMAs (DB = 12: 48 FMAs, packed by the compiler into 24 v_pk_fma_f32, per
//    4 reads); every lane of every wave is busy (41 planes padded to 48);
//  * the channel quarters' partial sums meet in LDS (the window's space, dead by then) and each wave
//    writes its share of the d planes.
// ----------------------------------------------------------------------------
template <int S, int DB, int NDH, int SIM>
__global__ __launch_bounds__(256 * NDH, (NDH == 1 ? 2 : 1)) void corr1d_tile_kernel(
    const float* __restrict__ fL, const float* __restrict__ fR, float* __restrict__ out,
    const float* __restrict__ inv, int C, int H, int W, int D) {
  constexpr int DP = 4 * DB * NDH, PADL = DP * S, RW = TX + PADL;
  constexpr int QR = RW / 4;                    // staged quads per channel
  constexpr int WIN = 4 + DB * S;               // floats of the fR window per thread
  static_assert((DB * S) % 4 == 0, "16-byte aligned window reads");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* const Rs = lds;                        // [C][RW]; column j <-> x = x0 - PADL + j
  const int x0 = blockIdx.x * TX, y = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cw = wave & 3, dh = wave >> 2;      // channel quarter, d half
  const int xg = lane & 15, dg = lane >> 4, d0 = (dh * 4 + dg) * DB;
  const long plane = (long)H * W;
  const float* const baseL = fL + (long)b * C * plane + (long)y * W;
  const float* const baseR = fR + (long)b * C * plane + (long)y * W;
  const int cq = (C + 3) / 4, c_lo = cw * cq, c_hi = min(C, c_lo + cq);

  float acc[DB][4];
#pragma unroll
  for (int i = 0; i < DB; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0.f;
  const int x = x0 + 4 * xg;
  const bool live = x < W;
  // branch-free channel walk (the host sends only C % 16 == 0 here: every quarter is whole groups of
  // four channels): a lane past the row's end reads the last quad of the row (its sums are never
  // stored); pointers advance by uniform increments, LDS reads take immediate offsets
  const float* lptr = baseL + (live ? x : W - 4) + (long)c_lo * plane;
  const float* rcur = Rs + 4 * xg + PADL - (d0 + DB) * S + c_lo * RW;      // 16-B aligned
  constexpr int LA = 4;                         // fL quads in flight ahead of their use
  const int nc = c_hi - c_lo;
  f32x4 lq[LA];
  // channels [c_from, c_to) of the quarter, groups of four
  auto compute = [&](int c_from, int c_to) __attribute__((always_inline)) {
    f32x4 wq[2][WIN / 4];                       // the window of the channel in hand and of the next one
#pragma unroll
    for (int k = 0; k < WIN / 4; ++k) wq[0][k] = *reinterpret_cast<const f32x4*>(rcur + 4 * k);
    for (int c4 = c_from; c4 < c_to; c4 += LA) {
      // the next group's fL quads (the last group re-reads itself: nothing past the tensor is touched)
      const float* lnext = lptr + (c4 + LA < nc ? (long)LA * plane : 0l);
#pragma unroll
      for (int u = 0; u < LA; ++u) {
        const f32x4 l = lq[u];
        lq[u] = *reinterpret_cast<const f32x4*>(lnext + (long)u * plane);
#pragma unroll
        for (int k = 0; k < WIN / 4; ++k)       // (the row past the last staged one: read, never used)
          wq[(u + 1) & 1][k] = *reinterpret_cast<const f32x4*>(rcur + (u + 1) * RW + 4 * k);
        float win[WIN];
#pragma unroll
        for (int k = 0; k < WIN / 4; ++k) {
          const f32x4 r = wq[u & 1][k];
          win[4 * k] = r.x; win[4 * k + 1] = r.y; win[4 * k + 2] = r.z; win[4 * k + 3] = r.w;
        }
#pragma unroll
        for (int i = 0; i < DB; ++i) {
          // output x = x0 + 4 xg + j pairs with fR column x - (d0 + i) S = window[j + (DB - i) S]
          acc[i][0] = fmaf(l.x, win[0 + (DB - i) * S], acc[i][0]);
          acc[i][1] = fmaf(l.y, win[1 + (DB - i) * S], acc[i][1]);
          acc[i][2] = fmaf(l.z, win[2 + (DB - i) * S], acc[i][2]);
          acc[i][3] = fmaf(l.w, win[3 + (DB - i) * S], acc[i][3]);
        }
      }
      lptr = lnext;
      rcur += LA * RW;
    }
  };

  // ---- stage the fR rows of this wave's channels (the d halves of a quarter split them) and compute
  // the channels that have arrived while the later loads are still in flight: the whole problem is
  // resident at once, so a load-everything-then-compute kernel would leave the memory system idle
  // while the chip multiplies and the ALUs idle while it loads
  {
    const int n = nc * QR;                      // quads of the quarter
    constexpr int NB = S == 1 ? 16 : 8;         // loads in flight per thread and batch (registers: S = 2 has the wider window)
#pragma unroll
    for (int u = 0; u < LA; ++u) lq[u] = *reinterpret_cast<const f32x4*>(lptr + (long)u * plane);
    int done = 0;                               // channels of the quarter multiplied so far
    for (int i0 = dh * 64 + lane; i0 - (dh * 64 + lane) < n; i0 += 64 * NDH * NB) {
      f32x4 v[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const int i = i0 + 64 * NDH * u;
        const int c = i / QR, k = i - c * QR;
        const int xr = x0 - PADL + 4 * k;
        v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (i < n && xr >= 0 && xr < W)         // W % 4 == 0 and xr % 4 == 0: a quad is all in or all out
          v[u] = *reinterpret_cast<const f32x4*>(baseR + (c_lo + c) * plane + xr);
      }
#pragma unroll
      for (int g4 = 0; g4 < NB; g4 += 4) {
#pragma unroll
        for (int u = g4; u < g4 + 4; ++u) {
          const int i = i0 + 64 * NDH * u;
          if (i < n) {
            const int c = i / QR, k = i - c * QR;
            *reinterpret_cast<f32x4*>(Rs + (c_lo + c) * RW + 4 * k) = v[u];
          }
        }
        if constexpr (NDH == 1) {
          // wave-private rows: LDS serves one wave's operations in order -- no workgroup barrier
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          // quads [0, first quad of the next store group) of the quarter are in LDS now
          const int upto = min(n, (i0 - lane) + 64 * (g4 + 4));
          const int ready = min(nc, (upto / QR) & ~(LA - 1));
          if (ready > done) { compute(done, ready); done = ready; }
        }
      }
    }
    if constexpr (NDH == 2) {
      __syncthreads();                          // the two d halves of a quarter staged it together
      compute(0, nc);
    } else if (done < nc) {
      compute(done, nc);
    }
  }

  // ---- the channel quarters' partial sums meet in LDS: P[cw][d][x]; then every wave finishes its share
  __syncthreads();                              // the window is dead
  constexpr int PW = TX + 4;                    // row pitch (floats)
  float* const P = lds;                         // [4][DP][PW]
#pragma unroll
  for (int i = 0; i < DB; ++i)
    *reinterpret_cast<f32x4*>(P + (cw * DP + d0 + i) * PW + 4 * xg) =
        f32x4{acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
  __syncthreads();
  if (!live) return;
  // wave (cw, dh) finishes planes (dh 4 + cw) DB + {dg, dg + 4, ...}: the four dg lanes of a column
  // step through the group together
#pragma unroll
  for (int t = 0; t < DB / 4; ++t) {
    const int d = (dh * 4 + cw) * DB + dg + 4 * t;
    if (d >= D) continue;
    f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int w = 0; w < 4; ++w) s4 += *reinterpret_cast<const f32x4*>(P + (w * DP + d) * PW + 4 * xg);
    if constexpr (SIM == DSM_SIM_COSINE) {
      float v[4] = {s4.x, s4.y, s4.z, s4.w};
      cos_scale4(v, inv, (long)gridDim.z * H * W, ((long)b * H + y) * W, x, d * S, W);
      s4 = f32x4{v[0], v[1], v[2], v[3]};
    }
    *reinterpret_cast<f32x4*>(out + (((long)b * D + d) * H + y) * W + x) = s4;
  }
}

// Any stride: one thread per output element (kept for strides other than 1, 2).
template <int SIM>
__global__ __launch_bounds__(256) void corr1d_fwd_generic_kernel(
    const float* __restrict__ fL, const float* __restrict__ fR, float* __restrict__ out,
    const float* __restrict__ inv, int C, int H, int W, int D, int S) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  const int y = blockIdx.y;
  const int b = blockIdx.z / D, d = blockIdx.z % D;
  if (x >= W) return;
  const int xs = x - d * S;
  float a = 0.f;
  if (xs >= 0) {
    const long plane = (long)H * W;
    const float* l = fL + (long)b * C * plane + (long)y * W + x;
    const float* r = fR + (long)b * C * plane + (long)y * W + xs;
    for (int c = 0; c < C; ++c) a = fmaf(l[c * plane], r[c * plane], a);
    if constexpr (SIM == DSM_SIM_COSINE) {
      const long row = ((long)b * H + y) * W;
      a *= inv[row + x] * inv[(long)(gridDim.z / D) * plane + row + xs];
    }
  }
  out[(((long)b * D + d) * H + y) * W + x] = a;
}

// AvgPool2d(k, stride 1, pad k/2) with the padding counted in the divisor
// (util_conv.py:82-85); also its own adjoint, so the backward reuses it.
__global__ __launch_bounds__(256) void box_filter_kernel(
    const float* __restrict__ src, float* __restrict__ dst, int H, int W, int k) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  const int y = blockIdx.y;
  if (x >= W) return;
  const float* p = src + (long)blockIdx.z * H * W;
  const int r = k / 2;
  float a = 0.f;
  for (int dy = -r; dy <= r; ++dy) {
    const int yy = y + dy;
    if (yy < 0 || yy >= H) continue;
    for (int dx = -r; dx <= r; ++dx) {
      const int xx = x + dx;
      if (xx >= 0 && xx < W) a += p[(long)yy * W + xx];
    }
  }
  dst[(long)blockIdx.z * H * W + (long)y * W + x] = a / (float)(k * k);
}

// The same for k = 3 on rows of W % 4 == 0: a thread owns four outputs of one (plane, row) and reads
// the three source rows as one 16-byte load + the two neighbours each (the source -- a correlation
// volume just written -- is cache-resident; the scalar kernel above spent 39 us on 20 MB).
__global__ __launch_bounds__(256) void box3_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                   long nplanes, int H, int W) {
  const int wq = W >> 2;
  const long n = nplanes * H * wq;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int xq = (int)(i % wq);
  const long row = i / wq;
  const int y = (int)(row % H);
  const float* p = src + row * W + 4 * xq;
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
    if (y + dy < 0 || y + dy >= H) continue;
    const float* q = p + (long)dy * W;
    const f32x4 v = *reinterpret_cast<const f32x4*>(q);
    const float l = xq > 0 ? q[-1] : 0.f, r = xq + 1 < wq ? q[4] : 0.f;
    a += f32x4{l + v.x + v.y, v.x + v.y + v.z, v.y + v.z + v.w, v.z + v.w + r};
  }
  *reinterpret_cast<f32x4*>(dst + row * W + 4 * xq) = a * (1.f / 9.f);
}

// Backward:
//   dfL[c,y,x ] = sum_i g[i,y,x]      * fR[c,y,x-i*s]
//   dfR[c,y,x'] = sum_i g[i,y,x'+i*s] * fL[c,y,x'+i*s]
// NORM (the cosine similarity; g is then g' of corr1d_sim_prep_bwd_kernel): the term of the norms' own
// gradient, dfL -= coef[0][b,y,x] fL, dfR -= coef[1][b,y,x] fR, coef = [2][B][H][W] written by the same pass.
template <bool NORM>
__global__ __launch_bounds__(256) void corr1d_bwd_kernel(
    const float* __restrict__ g, const float* __restrict__ fL, const float* __restrict__ fR,
    float* __restrict__ dfL, float* __restrict__ dfR, const float* __restrict__ coef, int C, int H, int W,
    int D, int S) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  const int y = blockIdx.y;
  const int bc = blockIdx.z;
  if (x >= W) return;
  const int b = bc / C;
  const long plane = (long)H * W;
  const float* gp = g + (long)b * D * plane + (long)y * W;
  const float* lrow = fL + (long)bc * plane + (long)y * W;
  const float* rrow = fR + (long)bc * plane + (long)y * W;
  const int dlim = min(D, W);
  float aL = 0.f, aR = 0.f;
  for (int i = 0; i < dlim; ++i) {
    const int sh = i * S;
    if (x - sh >= 0) aL = fmaf(gp[i * plane + x], rrow[x - sh], aL);
    if (x + sh < W) aR = fmaf(gp[i * plane + x + sh], lrow[x + sh], aR);
  }
  if constexpr (NORM) {
    const long pix = ((long)b * H + y) * W + x, npix = (long)(gridDim.z / C) * plane;
    aL -= coef[pix] * lrow[x];
    aR -= coef[npix + pix] * rrow[x];
  }
  dfL[(long)bc * plane + (long)y * W + x] = aL;
  dfR[(long)bc * plane + (long)y * W + x] = aR;
}

// ----------------------------------------------------------------------------
// Cosine similarity (Corr1d(simfun=nn.CosineSimilarity(dim=1)), util_conv.py:65): the pre-passes.
// ----------------------------------------------------------------------------
// inv[0][b,y,x] = a = 1 / max(||fL[b,:,y,x]||, eps), inv[1] = r, the same for fR: one launch.  A block owns 32
// items of either map -- an item is four columns (VEC: one 16-byte load per channel) or one -- and its eight
// thread rows take every eighth channel each (a map of 96 x 320 pixels is only 7680 quads: one thread per quad
// walking all channels leaves most of the chip idle); the rows' fp32 sums meet in LDS in a fixed order.
template <bool VEC>
__global__ __launch_bounds__(256) void corr1d_invnorm_kernel(
    const float* __restrict__ fL, const float* __restrict__ fR, float* __restrict__ inv, int C, long plane,
    long npix, float eps) {
  constexpr int V = VEC ? 4 : 1, NS = 8, NI = 256 / NS;
  __shared__ float part[NS][NI][V];
  const long n = npix / V;                       // items per map (VEC: plane % 4 == 0)
  const int li = threadIdx.x % NI, sl = threadIdx.x / NI;
  const long i = (long)blockIdx.x * NI + li;
  const bool live = i < 2 * n;
  const int m = i >= n;
  const long p = (i - m * n) * V;                // pixel index b * plane + y * W + x
  float s[V];
#pragma unroll
  for (int j = 0; j < V; ++j) s[j] = 0.f;
  if (live) {
    const long b = p / plane;
    const float* src = (m ? fR : fL) + b * C * plane + (p - b * plane);
    for (int c = sl; c < C; c += NS) {
      if constexpr (VEC) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + c * plane);
        s[0] = fmaf(v.x, v.x, s[0]); s[1] = fmaf(v.y, v.y, s[1]); s[2] = fmaf(v.z, v.z, s[2]); s[3] = fmaf(v.w, v.w, s[3]);
      } else {
        s[0] = fmaf(src[c * plane], src[c * plane], s[0]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) part[sl][li][j] = s[j];
  __syncthreads();
  if (sl != 0 || !live) return;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    float t = part[0][li][j];
#pragma unroll
    for (int k = 1; k < NS; ++k) t += part[k][li][j];
    inv[m * npix + p + j] = 1.f / fmaxf(sqrtf(t), eps);
  }
}

// Backward pre-pass: block = (b, y, 64 x), its four waves take every fourth plane each (their two sums meet in
// LDS in a fixed order); it reads g (the box-filtered cotangent) and the raw cosine map and writes
//   gp[i][x]   = g_i(x) a(x) r(x - i S)                          (what the dot-product backward then takes)
//   coef[0][x] = [||fL(x)|| >= eps] a(x)^2 sum_i g_i(x) raw_i(x)
//   coef[1][x] = [||fR(x)|| >= eps] r(x)^2 sum_i g_i(x + i S) raw_i(x + i S)
// A clamped norm is a constant: its pixel has coef = 0.  The norm counts as clamped where the stored inverse
// equals 1 / eps (float32): every norm below eps, and above it only one within a rounding of eps.
__global__ __launch_bounds__(256) void corr1d_sim_prep_bwd_kernel(
    const float* __restrict__ g, const float* __restrict__ raw, const float* __restrict__ inv,
    float* __restrict__ gp, float* __restrict__ coef, int H, int W, int D, int S, float eps) {
  __shared__ float part[4][2][64];
  const int lx = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int x = blockIdx.x * 64 + lx;
  const int y = blockIdx.y, b = blockIdx.z;
  const bool live = x < W;
  const long plane = (long)H * W, npix = (long)gridDim.z * plane;
  const long row = ((long)b * H + y) * W;
  const long base = (long)b * D * plane + (long)y * W;
  float a = 0.f, r = 0.f, tL = 0.f, tR = 0.f;
  if (live) {
    a = inv[row + x];
    r = inv[npix + row + x];
    const float* rinv = inv + npix + row;
    for (int i = sl; i < D; i += 4) {
      const int sh = i * S;
      const long o = base + i * plane;
      float v = 0.f;
      if (x - sh >= 0) {
        const float gi = g[o + x];
        v = gi * (a * rinv[x - sh]);
        tL = fmaf(gi, raw[o + x], tL);
      }
      gp[o + x] = v;
      if (x + sh < W) tR = fmaf(g[o + x + sh], raw[o + x + sh], tR);
    }
  }
  part[sl][0][lx] = tL;
  part[sl][1][lx] = tR;
  __syncthreads();
  if (sl != 0 || !live) return;
  tL = (part[0][0][lx] + part[1][0][lx]) + (part[2][0][lx] + part[3][0][lx]);
  tR = (part[0][1][lx] + part[1][1][lx]) + (part[2][1][lx] + part[3][1][lx]);
  const float clamp = 1.f / eps;
  coef[row + x] = a < clamp ? a * a * tL : 0.f;
  coef[npix + row + x] = r < clamp ? r * r * tR : 0.f;
}

// ----------------------------------------------------------------------------
// The tiled data gradient: stride 1 | 2, W % 4 == 0, 16-byte aligned pointers, D <= 96.
// Workgroup = (b, y, 64 x), 256 threads.  The naive kernel above re-reads the gradient rows once per
// channel (C D strided reads of g per row); here
//  * the D gradient rows of the tile go to LDS ONCE, twice over: G[i][k] = g_i(x0 + k) for dfL and the skewed
//    Gs[i][k] = g_i(x0 + k + i S) for dfR, so that both are read back as aligned 16-byte quads;
//  * per 32-channel chunk the fR window to the left, Rw[c][k] = fR[c][x0 - Dp S + k], and the fL window to
//    the right, Lw[c][k] = fL[c][x0 + k], k < 64 + Dp S (Dp = D rounded up to 4), as the r01 forward kernel
//    stages them;
//  * thread = (xg 0..15, cg 0..15) owns four columns of channels cg and cg + 16 for BOTH outputs and walks i in
//    groups of four: 4 + 4 gradient quads and, per channel, (4 + 4 S) / 4 quads of each window feed 64 FMAs.
// i ascends as in the naive kernel, so the sums round the same way.  No atomics.
// LDS: (2 Dp 64 + 2 * 32 * (64 + Dp S)) * 4 bytes: 81 KB at D = 81, S = 1; 115 KB at D = 96, S = 2 (the most).
// ----------------------------------------------------------------------------
constexpr int BT_CC = 32;    // channels per chunk
template <int S, bool NORM>
__global__ __launch_bounds__(256) void corr1d_bwd_tile_kernel(
    const float* __restrict__ g, const float* __restrict__ fL, const float* __restrict__ fR,
    float* __restrict__ dfL, float* __restrict__ dfR, const float* __restrict__ coef, int C, int H, int W,
    int D) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int WIN = 4 + 4 * S;                // floats of a window per thread and group of four planes
  const int Dp = (D + 3) & ~3, PADL = Dp * S, RW = TX + PADL;
  float* const G = lds;                         // [Dp][TX]
  float* const Gs = G + Dp * TX;                // [Dp][TX]
  float* const Rw = Gs + Dp * TX;               // [BT_CC][RW]; column k <-> x = x0 - PADL + k
  float* const Lw = Rw + BT_CC * RW;            // [BT_CC][RW]; column k <-> x = x0 + k
  const int x0 = blockIdx.x * TX, y = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, xg = tid & 15, cg = tid >> 4;
  const long plane = (long)H * W;
  const float* const gb = g + (long)b * D * plane + (long)y * W;

  // ---- the gradient rows, straight and skewed; planes D .. Dp - 1 and columns past the row are zero
  for (int i = tid; i < Dp * (TX / 4); i += 256) {
    const int d = i >> 4, q = i & 15;
    f32x4 v = {0.f, 0.f, 0.f, 0.f}, w = {0.f, 0.f, 0.f, 0.f};
    if (d < D) {
      const float* grow = gb + d * plane;
      const int x = x0 + 4 * q, xs = x + d * S;
      if (x < W) v = *reinterpret_cast<const f32x4*>(grow + x);        // W % 4 == 0: all in or all out
      if (xs + 3 < W) w = *reinterpret_cast<const f32x4u*>(grow + xs);
      else w = load4_guarded(grow, xs, W, false);
    }
    *reinterpret_cast<f32x4*>(G + d * TX + 4 * q) = v;
    *reinterpret_cast<f32x4*>(Gs + d * TX + 4 * q) = w;
  }

  const int x = x0 + 4 * xg;
  const int r4 = RW / 4;
  for (int c0 = 0; c0 < C; c0 += BT_CC) {
    const int cc = min(BT_CC, C - c0);
    __syncthreads();                            // the last chunk's windows are dead
    for (int i = tid; i < cc * r4; i += 256) {
      const int c = i / r4, k = i - c * r4;
      const long rowo = (((long)b * C + c0 + c) * H + y) * W;
      const int xr = x0 - PADL + 4 * k, xl = x0 + 4 * k;             // multiples of 4: a quad is all in or all out
      f32x4 vr = {0.f, 0.f, 0.f, 0.f}, vl = {0.f, 0.f, 0.f, 0.f};
      if (xr >= 0 && xr < W) vr = *reinterpret_cast<const f32x4*>(fR + rowo + xr);
      if (xl < W) vl = *reinterpret_cast<const f32x4*>(fL + rowo + xl);
      *reinterpret_cast<f32x4*>(Rw + c * RW + 4 * k) = vr;
      *reinterpret_cast<f32x4*>(Lw + c * RW + 4 * k) = vl;
    }
    __syncthreads();
    float aL[2][4], aR[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) aL[u][j] = aR[u][j] = 0.f;
    // (a thread whose channels lie past a partial chunk multiplies stale rows: its sums are never stored)
    for (int i0 = 0; i0 < Dp; i0 += 4) {
      f32x4 g4[4], s4[4];
#pragma unroll
      for (int ii = 0; ii < 4; ++ii) {
        g4[ii] = *reinterpret_cast<const f32x4*>(G + (i0 + ii) * TX + 4 * xg);
        s4[ii] = *reinterpret_cast<const f32x4*>(Gs + (i0 + ii) * TX + 4 * xg);
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int c = cg + 16 * u;
        const float* rp = Rw + c * RW + PADL + 4 * xg - (i0 + 4) * S;   // 16-byte aligned, >= row start
        const float* lp = Lw + c * RW + 4 * xg + i0 * S;                // last read column 63 + Dp S < RW
        float rw[WIN], lw[WIN];
#pragma unroll
        for (int k = 0; k < WIN / 4; ++k) {
          const f32x4 r = *reinterpret_cast<const f32x4*>(rp + 4 * k);
          const f32x4 l = *reinterpret_cast<const f32x4*>(lp + 4 * k);
          rw[4 * k] = r.x; rw[4 * k + 1] = r.y; rw[4 * k + 2] = r.z; rw[4 * k + 3] = r.w;
          lw[4 * k] = l.x; lw[4 * k + 1] = l.y; lw[4 * k + 2] = l.z; lw[4 * k + 3] = l.w;
        }
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
          // dfL column x + j pairs plane i0 + ii with fR column x + j - (i0 + ii) S = rw[j + (4 - ii) S],
          // dfR column x + j with g and fL at x + j + (i0 + ii) S = s4[ii][j], lw[j + ii S]
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            aL[u][j] = fmaf(g4[ii][j], rw[j + (4 - ii) * S], aL[u][j]);
            aR[u][j] = fmaf(s4[ii][j], lw[j + ii * S], aR[u][j]);
          }
        }
      }
    }
    if (x < W) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int c = cg + 16 * u;
        if (c >= cc) continue;
        f32x4 vL = {aL[u][0], aL[u][1], aL[u][2], aL[u][3]}, vR = {aR[u][0], aR[u][1], aR[u][2], aR[u][3]};
        if constexpr (NORM) {
          const long pix = ((long)b * H + y) * W + x, npix = (long)gridDim.z * plane;
          vL -= *reinterpret_cast<const f32x4*>(coef + pix) * *reinterpret_cast<const f32x4*>(Lw + c * RW + 4 * xg);
          vR -= *reinterpret_cast<const f32x4*>(coef + npix + pix) *
                *reinterpret_cast<const f32x4*>(Rw + c * RW + PADL + 4 * xg);
        }
        const long o = (((long)b * C + c0 + c) * H + y) * W + x;
        *reinterpret_cast<f32x4*>(dfL + o) = vL;
        *reinterpret_cast<f32x4*>(dfR + o) = vR;
      }
    }
  }
}

static int check_corr(const void* a, const void* b, const void* c, int B, int C, int H, int W,
                      int D, int stride, int ksize, int dtype) {
  DSM_REQUIRE(a && b && c, DSM_ERR_ARG);
  DSM_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && D > 0 && stride > 0, DSM_ERR_ARG);
  DSM_REQUIRE(ksize >= 1 && (ksize & 1) == 1, DSM_ERR_ARG);       // util_conv.py:83
  DSM_REQUIRE(dtype == DSM_F32, DSM_ERR_UNSUPPORTED);
  DSM_REQUIRE(H <= 65535 && (long)B * D <= 65535 && (long)B * C <= 65535, DSM_ERR_UNSUPPORTED);
  return DSM_OK;
}

// What the dsm_corr1d_sim_* entry points check on top: the similarity, and the extents the cosine passes
// index with ints (a pixel index b H W + y W + x, a shifted column x + i stride).
static int check_sim(int B, int H, int W, int D, int stride, int sim, float eps) {
  DSM_REQUIRE(sim == DSM_SIM_DOT || sim == DSM_SIM_COSINE, DSM_ERR_ARG);
  DSM_REQUIRE(sim == DSM_SIM_DOT || (eps > 0.f && eps < INFINITY), DSM_ERR_ARG);
  DSM_REQUIRE((long)B * H * W <= 0x7fffffffl && (long)W + (long)D * stride <= 0x7fffffffl, DSM_ERR_UNSUPPORTED);
  return DSM_OK;
}

// The branch dsm_corr1d_fwd takes: chosen here once, for the launch code and for dsm_corr1d_plan.
enum { CORR_TILE = 0, CORR_FWD = 1, CORR_GENERIC = 2 };
enum { CORR_NO_BOX = 0, CORR_BOX3 = 1, CORR_BOX = 2 };
struct CorrPlan {
  int kernel;        // CORR_*
  int ndh;           // tile kernel: d halves (1: D <= 48, 2: D <= 96)
  int vec;           // 16-byte global accesses (W % 4 == 0 and every pointer aligned)
  int box;           // CORR_*BOX*: what follows for ksize > 1
  size_t tile_lds;   // tile kernel: window or reduction bytes, whichever is larger (+ 4096 at launch)
};

// inv: the cosine similarity's inverse norms (NULL for the dot product); it counts among the pointers of `vec`.
static int pick_corr(const void* fL, const void* fR, const void* out, const void* tmp, const void* inv,
                     int B, int C, int H, int W, int D, int stride, int ksize, int dtype, CorrPlan* p) {
  int rc = check_corr(fL, fR, out, B, C, H, W, D, stride, ksize, dtype);
  if (rc != DSM_OK) return rc;
  DSM_REQUIRE(ksize == 1 || tmp, DSM_ERR_ARG);
  const void* raw = ksize > 1 ? tmp : out;
  const int ndg = (D + DB - 1) / DB;
  p->vec = (W % 4 == 0) && dsm_aligned16(fL) && dsm_aligned16(fR) && dsm_aligned16(raw) && dsm_aligned16(inv);
  // the tile kernel: the fR window of all channels in LDS at once; D <= 48 with four waves, D <= 96
  // with eight (two d halves per channel quarter)
  p->ndh = D <= 48 ? 1 : (D <= 96 ? 2 : 0);
  const int DP_ = 48 * p->ndh;
  const size_t win_lds = (size_t)C * (TX + DP_ * stride) * sizeof(float);
  const size_t red_lds = (size_t)4 * DP_ * (TX + 4) * sizeof(float);
  p->tile_lds = win_lds > red_lds ? win_lds : red_lds;
  if (p->vec && p->ndh && C % 16 == 0 && (stride == 1 || stride == 2) && p->tile_lds + 4096 <= 150 * 1024)
    p->kernel = CORR_TILE;
  else if ((stride == 1 || stride == 2) && ndg * 16 <= 256)
    p->kernel = CORR_FWD;
  else
    p->kernel = CORR_GENERIC;
  p->box = ksize == 1 ? CORR_NO_BOX : (ksize == 3 && p->vec && dsm_aligned16(out) ? CORR_BOX3 : CORR_BOX);
  return DSM_OK;
}

static void corr_plan_name(const CorrPlan& p, int stride, int sim, char* buf, int len) {
  const char* box = p.box == CORR_BOX3 ? "+box3" : (p.box == CORR_BOX ? "+box" : "");
  const char* pre = sim == DSM_SIM_COSINE ? "cos:" : "";
  if (p.kernel == CORR_TILE) snprintf(buf, (size_t)len, "%stile<%d,%d>%s", pre, stride, p.ndh, box);
  else if (p.kernel == CORR_FWD) snprintf(buf, (size_t)len, "%sfwd<%d>%s%s", pre, stride, p.vec ? "vec" : "scalar", box);
  else snprintf(buf, (size_t)len, "%sgeneric%s", pre, box);
}

extern "C" int dsm_corr1d_plan(const void* fL, const void* fR, const void* out, const void* tmp, int B,
                               int C, int H, int W, int D, int stride, int ksize, int dtype, char* buf,
                               int len) {
  DSM_REQUIRE(buf && len > 0, DSM_ERR_ARG);
  CorrPlan p;
  int rc = pick_corr(fL, fR, out, tmp, nullptr, B, C, H, W, D, stride, ksize, dtype, &p);
  if (rc != DSM_OK) return rc;
  corr_plan_name(p, stride, DSM_SIM_DOT, buf, len);
  return DSM_OK;
}

// The launches of a forward plan; SIM = DSM_SIM_COSINE: the inverse norms first, then the same kernels with
// the cosine epilogue.
template <int SIM>
static int corr_fwd_launch(const CorrPlan& plan, const void* fL, const void* fR, void* out, void* tmp,
                           void* inv, int B, int C, int H, int W, int D, int stride, int ksize, float eps,
                           hipStream_t s) {
  dsm_clear_stale_error();
  float* raw = (float*)(ksize > 1 ? tmp : out);
  const int ndg = (D + DB - 1) / DB;
  const int vec = plan.vec;
  const int NDH_ = plan.ndh;
  const size_t tile_lds = plan.tile_lds;
  if (SIM == DSM_SIM_COSINE) {
    const long plane = (long)H * W, npix = (long)B * plane;
    if (vec)
      hipLaunchKernelGGL(corr1d_invnorm_kernel<true>, dim3(dsm_cdiv(2 * (npix / 4), 32)), dim3(256), 0, s,
                         (const float*)fL, (const float*)fR, (float*)inv, C, plane, npix, eps);
    else
      hipLaunchKernelGGL(corr1d_invnorm_kernel<false>, dim3(dsm_cdiv(2 * npix, 32)), dim3(256), 0, s,
                         (const float*)fL, (const float*)fR, (float*)inv, C, plane, npix, eps);
  }
  if (plan.kernel == CORR_TILE) {
    dim3 grid(dsm_cdiv(W, TX), H, B);
#define DSM_CORR_TILE(S_, NDH__)                                                                     \
    do {                                                                                             \
      DSM_REQUIRE((dsm_allow_lds<corr1d_tile_kernel<S_, 12, NDH__, SIM>>(150 * 1024) == DSM_OK), DSM_ERR_LAUNCH); \
      hipLaunchKernelGGL((corr1d_tile_kernel<S_, 12, NDH__, SIM>), grid, dim3(256 * NDH__), tile_lds + 4096, s, /* + a row of slack */ \
                         (const float*)fL, (const float*)fR, raw, (const float*)inv, C, H, W, D);     \
    } while (0)
    if (stride == 1 && NDH_ == 1) DSM_CORR_TILE(1, 1);
    else if (stride == 1) DSM_CORR_TILE(1, 2);
    else if (NDH_ == 1) DSM_CORR_TILE(2, 1);
    else DSM_CORR_TILE(2, 2);
#undef DSM_CORR_TILE
  } else if (plan.kernel == CORR_FWD) {
    const int threads = ((ndg * 16 + 63) / 64) * 64;
    const size_t lds = (size_t)CC * (TX + TX + ndg * DB * stride) * sizeof(float);
    dim3 grid(dsm_cdiv(W, TX), H, B);
    if (stride == 1)
      hipLaunchKernelGGL((corr1d_fwd_kernel<1, SIM>), grid, dim3(threads), lds, s, (const float*)fL,
                         (const float*)fR, raw, (const float*)inv, C, H, W, D, vec);
    else
      hipLaunchKernelGGL((corr1d_fwd_kernel<2, SIM>), grid, dim3(threads), lds, s, (const float*)fL,
                         (const float*)fR, raw, (const float*)inv, C, H, W, D, vec);
  } else {
    dim3 grid(dsm_cdiv(W, 256), H, B * D);
    hipLaunchKernelGGL(corr1d_fwd_generic_kernel<SIM>, grid, dim3(256), 0, s, (const float*)fL,
                       (const float*)fR, raw, (const float*)inv, C, H, W, D, stride);
  }
  if (plan.box == CORR_BOX3) {
    const long n = (long)B * D * H * (W / 4);
    hipLaunchKernelGGL(box3_kernel, dim3(dsm_cdiv(n, 256)), dim3(256), 0, s, (const float*)raw, (float*)out,
                       (long)B * D, H, W);
  } else if (plan.box == CORR_BOX) {
    dim3 grid(dsm_cdiv(W, 256), H, B * D);
    hipLaunchKernelGGL(box_filter_kernel, grid, dim3(256), 0, s, (const float*)raw, (float*)out,
                       H, W, ksize);
  }
  return dsm_launch_status();
}

extern "C" int dsm_corr1d_fwd(const void* fL, const void* fR, void* out, void* tmp, int B, int C,
                              int H, int W, int D, int stride, int ksize, int dtype,
                              dsm_stream_t stream) {
  CorrPlan plan;
  int rc = pick_corr(fL, fR, out, tmp, nullptr, B, C, H, W, D, stride, ksize, dtype, &plan);
  if (rc != DSM_OK) return rc;
  return corr_fwd_launch<DSM_SIM_DOT>(plan, fL, fR, out, tmp, nullptr, B, C, H, W, D, stride, ksize, 0.f,
                                      (hipStream_t)stream);
}

extern "C" int dsm_corr1d_bwd(const void* grad_out, const void* fL, const void* fR, void* dfL,
                              void* dfR, void* tmp, int B, int C, int H, int W, int D, int stride,
                              int ksize, int dtype, dsm_stream_t stream) {
  int rc = check_corr(grad_out, fL, fR, B, C, H, W, D, stride, ksize, dtype);
  if (rc != DSM_OK) return rc;
  DSM_REQUIRE(dfL && dfR, DSM_ERR_ARG);
  DSM_REQUIRE(ksize == 1 || tmp, DSM_ERR_ARG);
  hipStream_t s = (hipStream_t)stream;
  dsm_clear_stale_error();
  const float* g = (const float*)grad_out;
  if (ksize > 1) {
    dim3 grid(dsm_cdiv(W, 256), H, B * D);
    hipLaunchKernelGGL(box_filter_kernel, grid, dim3(256), 0, s, g, (float*)tmp, H, W, ksize);
    g = (const float*)tmp;
  }
  dim3 grid(dsm_cdiv(W, 256), H, B * C);
  hipLaunchKernelGGL(corr1d_bwd_kernel<false>, grid, dim3(256), 0, s, g, (const float*)fL,
                     (const float*)fR, (float*)dfL, (float*)dfR, (const float*)nullptr, C, H, W, D, stride);
  return dsm_launch_status();
}

// ----------------------------------------------------------------------------
// The entry points with a similarity argument.
// ----------------------------------------------------------------------------
static int pick_corr_sim(const void* fL, const void* fR, const void* out, const void* raw, const void* inv,
                         int B, int C, int H, int W, int D, int stride, int ksize, int sim, float eps,
                         int dtype, CorrPlan* p) {
  int rc = check_corr(fL, fR, out, B, C, H, W, D, stride, ksize, dtype);
  if (rc != DSM_OK) return rc;
  rc = check_sim(B, H, W, D, stride, sim, eps);
  if (rc != DSM_OK) return rc;
  DSM_REQUIRE(sim == DSM_SIM_DOT || inv, DSM_ERR_ARG);
  return pick_corr(fL, fR, out, raw, sim == DSM_SIM_COSINE ? inv : nullptr, B, C, H, W, D, stride, ksize,
                   dtype, p);
}

extern "C" int dsm_corr1d_sim_fwd_plan(const void* fL, const void* fR, const void* out, const void* raw,
                                       const void* inv, int B, int C, int H, int W, int D, int stride,
                                       int ksize, int sim, float eps, int dtype, char* buf, int len) {
  DSM_REQUIRE(buf && len > 0, DSM_ERR_ARG);
  CorrPlan p;
  int rc = pick_corr_sim(fL, fR, out, raw, inv, B, C, H, W, D, stride, ksize, sim, eps, dtype, &p);
  if (rc != DSM_OK) return rc;
  corr_plan_name(p, stride, sim, buf, len);
  return DSM_OK;
}

extern "C" int dsm_corr1d_sim_fwd(const void* fL, const void* fR, void* out, void* raw, void* inv, int B,
                                  int C, int H, int W, int D, int stride, int ksize, int sim, float eps,
                                  int dtype, dsm_stream_t stream) {
  CorrPlan plan;
  int rc = pick_corr_sim(fL, fR, out, raw, inv, B, C, H, W, D, stride, ksize, sim, eps, dtype, &plan);
  if (rc != DSM_OK) return rc;
  if (sim == DSM_SIM_COSINE)
    return corr_fwd_launch<DSM_SIM_COSINE>(plan, fL, fR, out, raw, inv, B, C, H, W, D, stride, ksize, eps,
                                           (hipStream_t)stream);
  return corr_fwd_launch<DSM_SIM_DOT>(plan, fL, fR, out, raw, nullptr, B, C, H, W, D, stride, ksize, 0.f,
                                      (hipStream_t)stream);
}

// Workspace of dsm_corr1d_sim_bwd, segments of whole 256 bytes: [the box-filtered cotangent (B,D,H,W), ksize > 1]
// [g' (B,D,H,W), cosine] [coef (2,B,H,W), cosine].
static size_t ws_round(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

extern "C" size_t dsm_corr1d_sim_workspace_bytes(int B, int C, int H, int W, int D, int ksize, int sim) {
  (void)C;
  if (B <= 0 || H <= 0 || W <= 0 || D <= 0) return 0;
  const size_t map = ws_round((size_t)B * D * H * W * sizeof(float));
  size_t n = ksize > 1 ? map : 0;
  if (sim == DSM_SIM_COSINE) n += map + ws_round((size_t)2 * B * H * W * sizeof(float));
  return n;
}

enum { BWD_NAIVE = 0, BWD_TILE = 1 };
struct CorrBwdPlan {
  int kernel;          // BWD_*
  int box;             // CORR_*BOX*: the cotangent's box filter (its own adjoint), first
  int prep;            // cosine: corr1d_sim_prep_bwd_kernel in front
  size_t lds;          // tile kernel
  float *gbox, *gp, *coef;   // workspace segments (NULL where not used)
  const float* g;      // what the data-gradient kernel reads
};

static int pick_corr_bwd(const void* grad_out, const void* fL, const void* fR, const void* raw,
                         const void* inv, const void* dfL, const void* dfR, void* workspace, int B, int C,
                         int H, int W, int D, int stride, int ksize, int sim, float eps, int flags, int dtype,
                         CorrBwdPlan* p) {
  int rc = check_corr(grad_out, fL, fR, B, C, H, W, D, stride, ksize, dtype);
  if (rc != DSM_OK) return rc;
  rc = check_sim(B, H, W, D, stride, sim, eps);
  if (rc != DSM_OK) return rc;
  DSM_REQUIRE(dfL && dfR && (flags & ~DSM_CORR_BWD_NAIVE) == 0, DSM_ERR_ARG);
  DSM_REQUIRE(sim == DSM_SIM_DOT || (raw && inv), DSM_ERR_ARG);
  DSM_REQUIRE(workspace || dsm_corr1d_sim_workspace_bytes(B, C, H, W, D, ksize, sim) == 0, DSM_ERR_ARG);
  const size_t map = ws_round((size_t)B * D * H * W * sizeof(float));
  char* ws = (char*)workspace;
  p->gbox = p->gp = p->coef = nullptr;
  p->g = (const float*)grad_out;
  if (ksize > 1) { p->gbox = (float*)ws; ws += map; p->g = p->gbox; }
  p->prep = sim == DSM_SIM_COSINE;
  if (p->prep) { p->gp = (float*)ws; p->coef = (float*)(ws + map); p->g = p->gp; }
  p->box = ksize == 1 ? CORR_NO_BOX
                      : (ksize == 3 && W % 4 == 0 && dsm_aligned16(grad_out) && dsm_aligned16(p->gbox) ? CORR_BOX3 : CORR_BOX);
  // the tile kernel: the gradient rows twice and both windows of a 32-channel chunk in LDS
  const int Dp = (D + 3) & ~3;
  p->lds = ((size_t)2 * Dp * TX + (size_t)2 * BT_CC * (TX + (size_t)Dp * stride)) * sizeof(float);
  const bool aligned = dsm_aligned16(p->g) && dsm_aligned16(fL) && dsm_aligned16(fR) && dsm_aligned16(dfL) &&
                       dsm_aligned16(dfR) && dsm_aligned16(p->coef);
  p->kernel = (!(flags & DSM_CORR_BWD_NAIVE) && (stride == 1 || stride == 2) && W % 4 == 0 && aligned && D <= 96 &&
               p->lds <= 150 * 1024) ? BWD_TILE : BWD_NAIVE;
  return DSM_OK;
}

extern "C" int dsm_corr1d_sim_bwd_plan(const void* grad_out, const void* fL, const void* fR, const void* raw,
                                       const void* inv, const void* dfL, const void* dfR, const void* workspace,
                                       int B, int C, int H, int W, int D, int stride, int ksize, int sim,
                                       float eps, int flags, int dtype, char* buf, int len) {
  DSM_REQUIRE(buf && len > 0, DSM_ERR_ARG);
  CorrBwdPlan p;
  int rc = pick_corr_bwd(grad_out, fL, fR, raw, inv, dfL, dfR, (void*)workspace, B, C, H, W, D, stride, ksize,
                         sim, eps, flags, dtype, &p);
  if (rc != DSM_OK) return rc;
  const char* box = p.box == CORR_BOX3 ? "box3+" : (p.box == CORR_BOX ? "box+" : "");
  if (p.kernel == BWD_TILE) snprintf(buf, (size_t)len, "%s%sbwd_tile<%d>", box, p.prep ? "prep+" : "", stride);
  else snprintf(buf, (size_t)len, "%s%sbwd_naive", box, p.prep ? "prep+" : "");
  return DSM_OK;
}

extern "C" int dsm_corr1d_sim_bwd(const void* grad_out, const void* fL, const void* fR, const void* raw,
                                  const void* inv, void* dfL, void* dfR, void* workspace, int B, int C, int H,
                                  int W, int D, int stride, int ksize, int sim, float eps, int flags,
                                  int dtype, dsm_stream_t stream) {
  CorrBwdPlan p;
  int rc = pick_corr_bwd(grad_out, fL, fR, raw, inv, dfL, dfR, workspace, B, C, H, W, D, stride, ksize, sim,
                         eps, flags, dtype, &p);
  if (rc != DSM_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  dsm_clear_stale_error();
  if (p.box == CORR_BOX3) {
    const long n = (long)B * D * H * (W / 4);
    hipLaunchKernelGGL(box3_kernel, dim3(dsm_cdiv(n, 256)), dim3(256), 0, s, (const float*)grad_out, p.gbox,
                       (long)B * D, H, W);
  } else if (p.box == CORR_BOX) {
    dim3 grid(dsm_cdiv(W, 256), H, B * D);
    hipLaunchKernelGGL(box_filter_kernel, grid, dim3(256), 0, s, (const float*)grad_out, p.gbox, H, W, ksize);
  }
  if (p.prep) {
    dim3 grid(dsm_cdiv(W, 64), H, B);
    hipLaunchKernelGGL(corr1d_sim_prep_bwd_kernel, grid, dim3(256), 0, s,
                       (const float*)(ksize > 1 ? p.gbox : (const float*)grad_out), (const float*)raw,
                       (const float*)inv, p.gp, p.coef, H, W, D, stride, eps);
  }
  if (p.kernel == BWD_TILE) {
    dim3 grid(dsm_cdiv(W, TX), H, B);
#define DSM_CORR_BWD_TILE(S_, NORM_)                                                                 \
    do {                                                                                             \
      DSM_REQUIRE((dsm_allow_lds<corr1d_bwd_tile_kernel<S_, NORM_>>(150 * 1024) == DSM_OK), DSM_ERR_LAUNCH); \
      hipLaunchKernelGGL((corr1d_bwd_tile_kernel<S_, NORM_>), grid, dim3(256), p.lds, s, p.g,       \
                         (const float*)fL, (const float*)fR, (float*)dfL, (float*)dfR,               \
                         (const float*)p.coef, C, H, W, D);                                          \
    } while (0)
    if (stride == 1 && !p.prep) DSM_CORR_BWD_TILE(1, false);
    else if (stride == 1) DSM_CORR_BWD_TILE(1, true);
    else if (!p.prep) DSM_CORR_BWD_TILE(2, false);
    else DSM_CORR_BWD_TILE(2, true);
#undef DSM_CORR_BWD_TILE
  } else {
    dim3 grid(dsm_cdiv(W, 256), H, B * C);
    if (p.prep)
      hipLaunchKernelGGL(corr1d_bwd_kernel<true>, grid, dim3(256), 0, s, p.g, (const float*)fL, (const float*)fR,
                         (float*)dfL, (float*)dfR, (const float*)p.coef, C, H, W, D, stride);
    else
      hipLaunchKernelGGL(corr1d_bwd_kernel<false>, grid, dim3(256), 0, s, p.g, (const float*)fL, (const float*)fR,
                         (float*)dfL, (float*)dfR, (const float*)nullptr, C, H, W, D, stride);
  }
  return dsm_launch_status();
}

