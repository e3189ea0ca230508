// Result maps of a disparity map, on the device: the inverse of frames.hip.  From the fp32 map a network
// returns (and, for the error picture, the ground truth) to the bytes of the files a user keeps:
//   u16   KITTI's 16-bit encoding, value * 256, 0 = invalid (what Dataset_stereo(disp_png="kitti") reads)
//   u8    what the reference's submit() writes (stereo.py:174: cv2.imwrite of the float plane)
//   rgb   viridis against a fixed range, or against the image's own range as plt.imsave does
//   err   the KITTI devkit's log-scale error picture against ground truth, undilated
// The rules are stated per output in include/dsmnet_hip.h; every operation is a correctly rounded fp32
// or an integer one, so tests/encode_oracle.py restates them in numpy and compares bytes.
//
//   encode_range   (auto-range only) per (image, block): fminf / fmaxf over the finite, unmasked pixels
//                  of the window that the block sweeps, to workspace[image][block][2].  At most
//                  RANGE_BLOCKS blocks per image.
//   encode_rows    per (image, 256 groups of four consecutive output columns of one row): the inputs
//                  read once at the same element (16 bytes of disp / gt per lane, 4 of mask), every
//                  requested output computed from them and written with the widest store its address
//                  allows (8 B u16, 4 B u8, 12 B rgb / err per lane).  An rgb row is 3 * w bytes, so
//                  with w % 4 != 0 only some rows start on a dword: the choice is per thread, and the
//                  row's last group is always scalar.  With auto-range every block reduces its image's
//                  partials itself.  The viridis table is staged in LDS (one packed dword per entry).
// No atomics, no host read: two runs give the same bits, and both launches can be captured in a graph.
#include "common.hpp"
#include "viridis_lut.hpp"

#pragma clang fp contract(off)

namespace {

static_assert(sizeof(dsm_encode_args) == 104, "dsm_encode_args layout (ctypes mirror in _lib.py)");

constexpr int NT = 256;                    // threads of a block: one group of four columns each
constexpr int RANGE_BLOCKS = 256;          // most partial extremes per image: one per thread of encode_rows

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x3u __attribute__((ext_vector_type(3), aligned(4)));

struct Work {
  const float* disp;
  const float* gt;
  const unsigned char* mask;
  unsigned short* u16;
  unsigned char* u8;
  unsigned char* rgb;
  unsigned char* err;
  float* partial;                          // [b][nrange][2]: min, max
  int B, Hs, Ws, y0, x0, h, w;
  int G;                                   // groups of four columns in a window row
  int bpi;                                 // blocks of encode_rows per image
  int nrange;                              // blocks of encode_range per image (0: fixed range)
  int flip;
  float lo, hi;                            // the fixed range
};

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN

// Four consecutive OUTPUT columns x .. x + 3 of a window row.  `row` points at the window's first source
// column of that row; with flip, output column c reads row[w - 1 - c].  A group that lies inside the
// window whole is one 16-byte load (dword alignment is all gfx950 asks of it); the row's tail is scalar.
__device__ __forceinline__ void load4(const float* row, int x, int w, bool flip, float v[4]) {
  if (x + 3 < w) {
    const f32x4u q = *(const f32x4u*)(row + (flip ? w - 4 - x : x));
    if (flip) { v[0] = q.w; v[1] = q.z; v[2] = q.y; v[3] = q.x; }
    else      { v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = x + k < w ? row[flip ? w - 1 - x - k : x + k] : 0.f;
  }
}

__device__ __forceinline__ void load4(const unsigned char* row, int x, int w, bool flip, unsigned char v[4]) {
  const unsigned char* p = row + (flip ? w - 4 - x : x);
  if (x + 3 < w && ((uintptr_t)p & 3u) == 0) {
    const uint32_t q = *(const uint32_t*)p;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (unsigned char)(q >> (8 * (flip ? 3 - k : k)));
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = x + k < w ? row[flip ? w - 1 - x - k : x + k] : 0;
  }
}

// twelve bytes of four RGB pixels
__device__ __forceinline__ void store_rgb4(unsigned char* p, int n, const uint32_t c[4]) {
  if (n == 4 && ((uintptr_t)p & 3u) == 0) {
    u32x3u q;
    q.x = c[0] | (c[1] << 24);
    q.y = (c[1] >> 8) | (c[2] << 16);
    q.z = (c[2] >> 16) | (c[3] << 8);
    *(u32x3u*)p = q;
  } else {
    for (int k = 0; k < n; ++k) {
      p[3 * k] = (unsigned char)c[k];
      p[3 * k + 1] = (unsigned char)(c[k] >> 8);
      p[3 * k + 2] = (unsigned char)(c[k] >> 16);
    }
  }
}

// R | G << 8 | B << 16 of the devkit's error colours, bin k = [edge[k-1], edge[k])
__device__ __forceinline__ uint32_t error_colour(float n) {
  const uint32_t colour[10] = {49u | 54u << 8 | 149u << 16,   69u | 117u << 8 | 180u << 16,
                               116u | 173u << 8 | 209u << 16, 171u | 217u << 8 | 233u << 16,
                               224u | 243u << 8 | 248u << 16, 254u | 224u << 8 | 144u << 16,
                               253u | 174u << 8 | 97u << 16,  244u | 109u << 8 | 67u << 16,
                               215u | 48u << 8 | 39u << 16,   165u | 0u << 8 | 38u << 16};
  uint32_t c = colour[9];                  // n >= 16, and a NaN (no comparison below holds)
#pragma unroll
  for (int k = 8; k >= 0; --k)             // the upper edges 16 / 2 ... 1 / 16: the lowest that holds stays
    if (n < 0.0625f * (float)(1 << k)) c = colour[k];
  return c;
}

__global__ __launch_bounds__(NT) void encode_range(const Work K) {
  __shared__ float s_lo[NT / 64], s_hi[NT / 64];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / K.nrange, blk = blockIdx.x - b * K.nrange;
  const int per = K.h * K.G;               // groups of one image (< 2^31: checked by the host)
  float lo = INFINITY, hi = -INFINITY;
  for (int gi = blk * NT + tid; gi < per; gi += K.nrange * NT) {
    const int y = gi / K.G, x = (gi - y * K.G) * 4;
    const long src = ((long)b * K.Hs + K.y0 + y) * K.Ws + K.x0;
    float d[4];
    unsigned char m[4] = {1, 1, 1, 1};
    load4(K.disp + src, x, K.w, false, d);
    if (K.mask) load4(K.mask + src, x, K.w, false, m);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (x + k < K.w && m[k] != 0 && finite_f(d[k])) {
        lo = fminf(lo, d[k]);
        hi = fmaxf(hi, d[k]);
      }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o, 64));
    hi = fmaxf(hi, __shfl_xor(hi, o, 64));
  }
  if (tid % 64 == 0) { s_lo[tid / 64] = lo; s_hi[tid / 64] = hi; }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 1; k < NT / 64; ++k) { lo = fminf(lo, s_lo[k]); hi = fmaxf(hi, s_hi[k]); }
    K.partial[2 * (long)blockIdx.x] = lo;
    K.partial[2 * (long)blockIdx.x + 1] = hi;
  }
}

__global__ __launch_bounds__(NT) void encode_rows(const Work K) {
  __shared__ uint32_t s_lut[DSM_VIRIDIS_ENTRIES];
  __shared__ float s_lo[NT / 64], s_hi[NT / 64];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / K.bpi, blk = blockIdx.x - b * K.bpi;
  float lo = K.lo, hi = K.hi;
  if (K.rgb) {
    static_assert(DSM_VIRIDIS_ENTRIES == NT, "one table entry per thread");
    s_lut[tid] = (uint32_t)dsm_viridis_lut[3 * tid] | ((uint32_t)dsm_viridis_lut[3 * tid + 1] << 8) |
                 ((uint32_t)dsm_viridis_lut[3 * tid + 2] << 16);
    if (K.nrange) {                        // the image's extremes from encode_range's partials
      lo = INFINITY; hi = -INFINITY;
      if (tid < K.nrange) {
        lo = K.partial[2 * ((long)b * K.nrange + tid)];
        hi = K.partial[2 * ((long)b * K.nrange + tid) + 1];
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
      }
      if (tid % 64 == 0) { s_lo[tid / 64] = lo; s_hi[tid / 64] = hi; }
    }
    __syncthreads();
    if (K.nrange) {
      lo = s_lo[0]; hi = s_hi[0];
#pragma unroll
      for (int k = 1; k < NT / 64; ++k) { lo = fminf(lo, s_lo[k]); hi = fmaxf(hi, s_hi[k]); }
    }
  }
  const int gi = blk * NT + tid;
  if (gi >= K.h * K.G) return;             // after the block's only barrier
  const int y = gi / K.G, x = (gi - y * K.G) * 4;
  const int w = K.w, n = min(4, w - x);
  const long src = ((long)b * K.Hs + K.y0 + y) * K.Ws + K.x0;
  const long o = ((long)b * K.h + y) * w + x;
  const bool flip = K.flip != 0;
  float d[4], g[4] = {0.f, 0.f, 0.f, 0.f};
  unsigned char m[4] = {1, 1, 1, 1};
  load4(K.disp + src, x, w, flip, d);
  if (K.gt && K.err) load4(K.gt + src, x, w, flip, g);
  if (K.mask) load4(K.mask + src, x, w, flip, m);
  bool ok[4];                              // the pixel carries a value: unmasked and finite
#pragma unroll
  for (int k = 0; k < 4; ++k) ok[k] = m[k] != 0 && finite_f(d[k]);

  if (K.u16) {
    unsigned short q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      q[k] = ok[k] ? (unsigned short)fminf(fmaxf(rintf(d[k] * 256.0f), 1.0f), 65535.0f) : 0;
    unsigned short* p = K.u16 + o;
    if (n == 4 && ((uintptr_t)p & 7u) == 0) {
      u32x2 v;
      v.x = (uint32_t)q[0] | ((uint32_t)q[1] << 16);
      v.y = (uint32_t)q[2] | ((uint32_t)q[3] << 16);
      *(u32x2*)p = v;
    } else {
      for (int k = 0; k < n; ++k) p[k] = q[k];
    }
  }
  if (K.u8) {
    unsigned char q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {          // convertTo(CV_8U): saturate(rint(d)); +Inf saturates too
      const bool carries = m[k] != 0 && d[k] == d[k];
      q[k] = carries ? (unsigned char)fminf(fmaxf(rintf(d[k]), 0.0f), 255.0f) : 0;
    }
    unsigned char* p = K.u8 + o;
    if (n == 4 && ((uintptr_t)p & 3u) == 0) {
      *(uint32_t*)p = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
    } else {
      for (int k = 0; k < n; ++k) p[k] = q[k];
    }
  }
  if (K.rgb) {
    uint32_t c[4];
    const float span = hi - lo;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float v = ((d[k] - lo) / span) * 256.0f;
      // hi == lo: entry 0 everywhere; below lo (and a NaN of an overflowing range): 0; 256 and above: 255
      const int idx = (hi == lo || !(v >= 0.0f)) ? 0 : (v >= 256.0f ? 255 : (int)v);
      c[k] = ok[k] ? s_lut[idx] : 0u;
    }
    store_rgb4(K.rgb + 3 * o, n, c);
  }
  if (K.err) {
    uint32_t c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool scored = m[k] != 0 && finite_f(g[k]) && g[k] > 0.0f;
      const float e = fabsf(g[k] - d[k]);
      // a NaN prediction makes both operands NaN, an infinite one both infinite: the last bin
      const float nrm = fminf(e / 3.0f, (e / g[k]) / 0.05f);
      c[k] = scored ? error_colour(nrm) : 0u;
    }
    store_rgb4(K.err + 3 * o, n, c);
  }
}

static bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return a && b && pa < pb + nb && pb < pa + na;
}

static int range_blocks(int h, int w) {
  const long per = (long)h * dsm_cdiv(w, 4);
  const long need = (per + NT - 1) / NT;
  return (int)(need < RANGE_BLOCKS ? need : RANGE_BLOCKS);
}

}  // namespace

extern "C" size_t dsm_disp_encode_workspace_bytes(int B, int h, int w) {
  if (B <= 0 || h <= 0 || w <= 0) return 0;
  return (size_t)B * range_blocks(h, w) * 2 * sizeof(float);
}

extern "C" int dsm_disp_encode(const dsm_encode_args* a, dsm_stream_t stream) {
  DSM_REQUIRE(a && a->disp, DSM_ERR_ARG);
  DSM_REQUIRE(a->u16 || a->u8 || a->rgb || a->err, DSM_ERR_ARG);
  DSM_REQUIRE(!a->err || a->gt, DSM_ERR_ARG);
  DSM_REQUIRE((a->flags & ~(DSM_ENCODE_FLIP | DSM_ENCODE_AUTO_RANGE)) == 0, DSM_ERR_ARG);
  const bool autorange = a->rgb && (a->flags & DSM_ENCODE_AUTO_RANGE);
  DSM_REQUIRE(!autorange || a->workspace, DSM_ERR_ARG);
  DSM_REQUIRE(a->B > 0 && a->Hs > 0 && a->Ws > 0 && a->h > 0 && a->w > 0, DSM_ERR_ARG);
  DSM_REQUIRE(a->y0 >= 0 && a->x0 >= 0 && a->y0 <= a->Hs - a->h && a->x0 <= a->Ws - a->w, DSM_ERR_ARG);
  if (a->rgb && !autorange)
    DSM_REQUIRE(fabsf(a->vmin) <= 3.402823466e38f && fabsf(a->vmax) <= 3.402823466e38f && a->vmax >= a->vmin,
                DSM_ERR_ARG);
  const long rows = (long)a->B * a->Hs;
  const bool fits = rows < (1L << 31) && rows * a->Ws < (1L << 31);
  if (fits) {                              // byte extents that fit: any overlap of an output with an input
    const size_t ns = (size_t)rows * a->Ws, nd = (size_t)a->B * a->h * a->w;
    const void* in[3] = {a->disp, a->gt, a->mask};
    const size_t nin[3] = {ns * 4, ns * 4, ns};
    const void* out[5] = {a->u16, a->u8, a->rgb, a->err, autorange ? a->workspace : nullptr};
    const size_t nout[5] = {nd * 2, nd, nd * 3, nd * 3, dsm_disp_encode_workspace_bytes(a->B, a->h, a->w)};
    for (int i = 0; i < 5; ++i)
      for (int j = 0; j < 3; ++j) DSM_REQUIRE(!overlap(out[i], nout[i], in[j], nin[j]), DSM_ERR_ARG);
    for (int i = 0; i < 4; ++i) DSM_REQUIRE(!overlap(out[i], nout[i], out[4], nout[4]), DSM_ERR_ARG);
  }
  DSM_REQUIRE((((uintptr_t)a->disp | (uintptr_t)a->gt | (autorange ? (uintptr_t)a->workspace : 0)) & 3u) == 0,
              DSM_ERR_ALIGN);
  DSM_REQUIRE(((uintptr_t)a->u16 & 1u) == 0, DSM_ERR_ALIGN);
  DSM_REQUIRE(fits, DSM_ERR_UNSUPPORTED);                                     // 32-bit element indices
  Work K;
  K.disp = (const float*)a->disp; K.gt = (const float*)a->gt; K.mask = (const unsigned char*)a->mask;
  K.u16 = (unsigned short*)a->u16; K.u8 = (unsigned char*)a->u8;
  K.rgb = (unsigned char*)a->rgb; K.err = (unsigned char*)a->err;
  K.partial = autorange ? (float*)a->workspace : nullptr;
  K.B = a->B; K.Hs = a->Hs; K.Ws = a->Ws; K.y0 = a->y0; K.x0 = a->x0; K.h = a->h; K.w = a->w;
  K.G = dsm_cdiv(a->w, 4);
  K.bpi = dsm_cdiv((long)a->h * K.G, NT);
  K.nrange = autorange ? range_blocks(a->h, a->w) : 0;
  K.flip = (a->flags & DSM_ENCODE_FLIP) ? 1 : 0;
  K.lo = a->vmin; K.hi = a->vmax;
  dsm_clear_stale_error();
  if (autorange)
    hipLaunchKernelGGL(encode_range, dim3((unsigned)((long)a->B * K.nrange)), dim3(NT), 0, (hipStream_t)stream, K);
  hipLaunchKernelGGL(encode_rows, dim3((unsigned)((long)a->B * K.bpi)), dim3(NT), 0, (hipStream_t)stream, K);
  return dsm_launch_status();
}
