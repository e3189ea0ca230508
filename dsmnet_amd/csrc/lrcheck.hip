// Left-right consistency check and background hole fill of a disparity map, on the product path
// (utils/imwrap.py:37-72 imwrap_BCHW with fliplr=True at LeftTop [0,0], scale 1, as losses/loss.py:451-452
// calls it; losses/loss.py:393-404 weight_common).  The -mask objectives of selfsup.hip compute the same
// two quantities per pixel as a term of a scalar loss; here they are the result.
//
//   lr_check_tiles   per (image, 16x64 tile), four consecutive columns per thread: disp read once (16
//                    bytes per lane where the rows allow it), the other view's map gathered at the flip
//                    grid (sixteen taps per thread in flight together), wrap / weight / mask / masked
//                    written with plain stores.  One launch.
//   fill_rows        one workgroup per (image, row).  A forward sweep over 256-column chunks copies the
//                    valid pixels and leaves, in every invalid one, the value of the nearest valid column
//                    to its left; a backward sweep finds the nearest valid value to the right and keeps
//                    the smaller.  Inside a wave the neighbour is a bit scan of the 64-bit validity ballot
//                    and one shuffle; across waves and chunks it is carried through LDS.  The row's
//                    "has a valid pixel" flag goes to the workspace.
//   fill_empty_rows  one workgroup per (image, row), at once done unless the row is empty: the nearest
//                    non-empty rows above and below are found from the flags, the row is their fminf.
// No atomics, no host read: two runs give the same bits, and all of it can be captured in a graph.
// The value of an invalid pixel is never loaded, so nothing of it can reach the output.
#include "common.hpp"

namespace {

constexpr int TH = 16, TW = 64;            // tile: 1024 pixels, four consecutive columns per thread
static_assert(sizeof(dsm_lrcheck_args) == 80, "dsm_lrcheck_args layout (ctypes mirror in _lib.py)");

struct Work {
  const float* disp;
  const float* other;
  float* wrap;
  float* weight;
  unsigned char* mask;
  float* masked;
  int B, H, W, nty, ntx, per;              // per = tiles of one image
  int vec;                                 // 16-byte loads of disp and stores of the fp32 outputs, 4-byte of mask
  int right_frame;                         // `other` is read at column W - 1 - x
  float delt, factor, threshold;
};

// grid_sample's bilinear tap set (bilinear, zeros, align_corners=False) at the flip grid of
// imwrap_BCHW(.., fliplr=True, LeftTop [0,0], scale 1): x coordinate -(linspace(-1, 1, W)[x] - d * 2 / (W - 1))
struct Taps {
  int x0, y0;                              // the nw tap; dereference behind i00..i11 only
  float nw, ne, sw, se, ix;
  bool i00, i01, i10, i11;
};

__device__ __forceinline__ Taps flip_grid_taps(float d, int x, int y, int H, int W) {
  Taps t;
  const float gx = -(linspace_at(-1.f, 1.f, W, x) - d * 2.0f / (float)(W - 1));
  const float gy = linspace_at(-1.f, 1.f, H, y);
  const float ix = ((gx + 1.f) * (float)W - 1.f) / 2.f;
  const float iy = ((gy + 1.f) * (float)H - 1.f) / 2.f;
  const float fx = floorf(ix), fy = floorf(iy);
  // wild disparities: clamp before the int conversion (the taps then fall outside, as in torch)
  t.x0 = (int)fminf(fmaxf(fx, -2.f), (float)W + 1.f);
  t.y0 = (int)fminf(fmaxf(fy, -2.f), (float)H + 1.f);
  const float wx1 = ix - fx, wx0 = (fx + 1.f) - ix, wy1 = iy - fy, wy0 = (fy + 1.f) - iy;
  const bool inx0 = t.x0 >= 0 && t.x0 < W, inx1 = t.x0 + 1 >= 0 && t.x0 + 1 < W;
  const bool iny0 = t.y0 >= 0 && t.y0 < H, iny1 = t.y0 + 1 >= 0 && t.y0 + 1 < H;
  t.i00 = iny0 && inx0; t.i01 = iny0 && inx1; t.i10 = iny1 && inx0; t.i11 = iny1 && inx1;
  t.nw = wx0 * wy0; t.ne = wx1 * wy0; t.sw = wx0 * wy1; t.se = wx1 * wy1;
  t.ix = ix;
  return t;
}

__device__ __forceinline__ float weight_of(float delta) {              // loss.py:393-404
  return delta < 1.f ? 1.f : (delta < 3.f ? 1.f - (delta - 1.f) * (0.99f / 2.f) : 0.01f);
}

__device__ __forceinline__ void store4(float* row, int x, int W, bool vec, const float v[4]) {
  if (vec) {
    f32x4 q;
    q.x = v[0]; q.y = v[1]; q.z = v[2]; q.w = v[3];
    *(f32x4*)(row + x) = q;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (x + k < W) row[x + k] = v[k];
  }
}

__global__ __launch_bounds__(256) void lr_check_tiles(const Work K) {
  const int tid = threadIdx.x;
  const int b = blockIdx.x / K.per, local = blockIdx.x - b * K.per;
  const int H = K.H, W = K.W;
  const int y = (local / K.ntx) * TH + tid / (TW / 4);
  const int x = (local % K.ntx) * TW + (tid % (TW / 4)) * 4;
  if (y >= H || x >= W) return;
  const long plane = (long)H * W;
  const long o = (long)b * plane + (long)y * W;          // the pixel row
  float d[4];
  if (K.vec) {                                           // W % 4 == 0: the four pixels are inside together
    const f32x4 q = *(const f32x4*)(K.disp + o + x);
    d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = x + k < W ? K.disp[o + x + k] : 0.f;
  }
  const float* src = K.other + (long)b * plane;
  Taps T[4];
  float t[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {                          // the sixteen taps in flight together
    T[k] = flip_grid_taps(d[k], min(x + k, W - 1), y, H, W);
    // the column of a tap in `other` as it lies in memory: mirrored, or the right camera's own frame
    const int c0 = K.right_frame ? W - 1 - T[k].x0 : T[k].x0;
    const int c1 = K.right_frame ? c0 - 1 : c0 + 1;
    const long r0 = (long)T[k].y0 * W, r1 = r0 + W;
    t[k][0] = T[k].i00 ? src[r0 + c0] : 0.f;
    t[k][1] = T[k].i01 ? src[r0 + c1] : 0.f;
    t[k][2] = T[k].i10 ? src[r1 + c0] : 0.f;
    t[k][3] = T[k].i11 ? src[r1 + c1] : 0.f;
  }
  float wr[4], wt[4], md[4];
  unsigned char m[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float v = 0.f;                                       // torch's order: nw, ne, sw, se; `+ delt` inside only
    if (T[k].i00) v += (t[k][0] + K.delt) * T[k].nw;
    if (T[k].i01) v += (t[k][1] + K.delt) * T[k].ne;
    if (T[k].i10) v += (t[k][2] + K.delt) * T[k].sw;
    if (T[k].i11) v += (t[k][3] + K.delt) * T[k].se;
    const float delta = fabsf(d[k] - v) / K.factor;
    // a sample that is half out of the image is a zero-padded average, not a measurement
    const bool ok = delta < K.threshold && T[k].ix >= 0.f && T[k].ix <= (float)(W - 1);
    wr[k] = v;
    wt[k] = weight_of(delta);
    m[k] = ok ? 1 : 0;
    md[k] = ok ? d[k] : 0.f;
  }
  if (K.wrap) store4(K.wrap + o, x, W, K.vec, wr);
  if (K.weight) store4(K.weight + o, x, W, K.vec, wt);
  if (K.masked) store4(K.masked + o, x, W, K.vec, md);
  if (K.mask) {
    if (K.vec) {
      *(uint32_t*)(K.mask + o + x) = (uint32_t)m[0] | ((uint32_t)m[1] << 8) | ((uint32_t)m[2] << 16) |
                                     ((uint32_t)m[3] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (x + k < W) K.mask[o + x + k] = m[k];
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// hole fill
// ---------------------------------------------------------------------------------------------------
constexpr int CH = 256;                    // columns of one chunk: one per thread, four waves

struct Fill {
  const float* disp;
  const unsigned char* mask;
  float* out;
  int* rowflag;                            // [b][y]: the row has a valid pixel
  int B, H, W;
};

__global__ __launch_bounds__(CH) void fill_rows(const Fill K) {
  // per wave of a chunk: any valid lane, and the value a neighbouring wave needs (forward: of the last
  // valid lane; backward: of the first).  Two sets: a chunk writes the set its parity names, so one
  // barrier per chunk is enough (nobody can be two chunks ahead of a reader).
  __shared__ int s_has[2][4];
  __shared__ float s_val[2][4];
  __shared__ int s_lo[2][4], s_hi[2][4];
  const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64;
  const int W = K.W;
  const long o = (long)blockIdx.x * W;                   // blockIdx.x = b * H + y
  const int nch = (W + CH - 1) / CH;

  // forward: valid pixels copied, invalid ones get the nearest valid value on their left (0: none yet)
  float carry = 0.f;                                     // of the chunks (and waves) before: the same in
  int first = -1, last = -1;                             // every thread.  first / last valid column.
  for (int c = 0; c < nch; ++c) {
    const int x = c * CH + tid, p = c & 1;
    const bool valid = x < W && K.mask[o + x] != 0;
    const float v = valid ? K.disp[o + x] : 0.f;         // an invalid pixel's value is never loaded
    const unsigned long long bal = __ballot(valid);
    const unsigned long long below = bal & ((2ull << lane) - 1ull);          // lanes <= this one
    const float left = __shfl(v, below ? 63 - __clzll((long long)below) : 0, 64);
    const float wlast = __shfl(v, bal ? 63 - __clzll((long long)bal) : 0, 64);
    if (lane == 0) {
      s_has[p][wave] = bal != 0;
      s_val[p][wave] = wlast;
      s_lo[p][wave] = bal ? c * CH + wave * 64 + __ffsll((long long)bal) - 1 : -1;
      s_hi[p][wave] = bal ? c * CH + wave * 64 + 63 - __clzll((long long)bal) : -1;
    }
    __syncthreads();
    float in = carry;                                    // what reaches this wave from its left
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (s_has[p][w]) {
        if (w < wave) in = s_val[p][w];
        carry = s_val[p][w];
        if (first < 0) first = s_lo[p][w];
        last = s_hi[p][w];
      }
    }
    if (x < W) K.out[o + x] = below ? left : in;
  }
  __syncthreads();                                       // the sets are reused from parity 0
  if (tid == 0) K.rowflag[blockIdx.x] = first >= 0;
  if (first < 0) return;                                 // an empty row: fill_empty_rows writes it

  // backward: out[x] of a valid pixel is its value, of an invalid one the value on its left
  carry = 0.f;
  for (int c = nch - 1, it = 0; c >= 0; --c, ++it) {
    const int x = c * CH + tid, p = it & 1;
    const bool valid = x < W && K.mask[o + x] != 0;
    const bool mine = x < W && (valid || x > first);     // out[x] holds a value of a valid pixel
    const float v = mine ? K.out[o + x] : 0.f;
    const unsigned long long bal = __ballot(valid);
    const unsigned long long above = bal >> lane;                           // lanes >= this one
    const float right = __shfl(v, above ? lane + __ffsll((long long)above) - 1 : 0, 64);
    const float wfirst = __shfl(v, bal ? __ffsll((long long)bal) - 1 : 0, 64);
    if (lane == 0) {
      s_has[p][wave] = bal != 0;
      s_val[p][wave] = wfirst;
    }
    __syncthreads();
    float in = carry;                                    // what reaches this wave from its right
#pragma unroll
    for (int w = 3; w >= 0; --w) {
      if (s_has[p][w]) {
        if (w > wave) in = s_val[p][w];
        carry = s_val[p][w];
      }
    }
    if (x < W && !valid) {
      const float r = above ? right : in;
      const bool hasl = x > first, hasr = x < last;
      K.out[o + x] = hasl && hasr ? fminf(v, r) : (hasl ? v : r);
    }
  }
}

__global__ __launch_bounds__(CH) void fill_empty_rows(const Fill K) {
  __shared__ int s_near[2][4];
  const int H = K.H, W = K.W;
  const int b = blockIdx.x / H, y = blockIdx.x - b * H;
  const int* flag = K.rowflag + (long)b * H;
  if (flag[y]) return;
  const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64;
  // the nearest non-empty row above (dir 0) and below (dir 1): 256 rows looked at per step
  int near[2] = {-1, -1};
  for (int dir = 0; dir < 2; ++dir) {
    const int step = dir ? 1 : -1;
    int it = 0;
    for (int base = y + step; base >= 0 && base < H; base += step * CH, ++it) {
      const int r = base + step * tid, p = it & 1;
      const bool hit = r >= 0 && r < H && flag[r] != 0;
      const unsigned long long bal = __ballot(hit);
      if (lane == 0) s_near[p][wave] = bal ? wave * 64 + __ffsll((long long)bal) - 1 : CH;
      __syncthreads();
      const int m = min(min(s_near[p][0], s_near[p][1]), min(s_near[p][2], s_near[p][3]));
      if (m < CH) {
        near[dir] = base + step * m;
        break;
      }
    }
    __syncthreads();                                     // the next search starts at parity 0 again
  }
  const float* up = near[0] >= 0 ? K.out + ((long)b * H + near[0]) * W : nullptr;
  const float* dn = near[1] >= 0 ? K.out + ((long)b * H + near[1]) * W : nullptr;
  float* row = K.out + (long)blockIdx.x * W;
  for (int x = tid; x < W; x += CH)
    row[x] = up && dn ? fminf(up[x], dn[x]) : (up ? up[x] : (dn ? dn[x] : 0.f));
}

static bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + nb && pb < pa + na;
}

}  // namespace

extern "C" int dsm_lr_check(const dsm_lrcheck_args* a, dsm_stream_t stream) {
  DSM_REQUIRE(a && a->disp && a->other, DSM_ERR_ARG);
  DSM_REQUIRE(a->wrap || a->weight || a->mask || a->masked, DSM_ERR_ARG);
  DSM_REQUIRE(a->B > 0 && a->H > 1 && a->W > 1, DSM_ERR_ARG);                 // imwrap.py:48
  DSM_REQUIRE(a->factor > 0.f && a->factor <= 3.402823466e38f, DSM_ERR_ARG);
  DSM_REQUIRE(a->threshold >= -3.402823466e38f && a->threshold <= 3.402823466e38f, DSM_ERR_ARG);
  DSM_REQUIRE((a->flags & ~DSM_LRCHECK_OTHER_RIGHT_FRAME) == 0, DSM_ERR_ARG);
  const uintptr_t maps = (uintptr_t)a->disp | (uintptr_t)a->other | (uintptr_t)a->wrap |
                         (uintptr_t)a->weight | (uintptr_t)a->masked;
  DSM_REQUIRE((maps & 3u) == 0, DSM_ERR_ALIGN);
  Work K;
  K.B = a->B; K.H = a->H; K.W = a->W;
  K.nty = dsm_cdiv(a->H, TH); K.ntx = dsm_cdiv(a->W, TW);
  const long per = (long)K.nty * K.ntx;
  DSM_REQUIRE(per * a->B < (1L << 31), DSM_ERR_UNSUPPORTED);                  // the grid's x extent
  K.per = (int)per;
  K.disp = (const float*)a->disp; K.other = (const float*)a->other;
  K.wrap = (float*)a->wrap; K.weight = (float*)a->weight;
  K.mask = (unsigned char*)a->mask; K.masked = (float*)a->masked;
  K.vec = (a->W % 4 == 0 && dsm_aligned16(a->disp) && dsm_aligned16(a->wrap) && dsm_aligned16(a->weight) &&
           dsm_aligned16(a->masked) && ((uintptr_t)a->mask & 3u) == 0) ? 1 : 0;
  K.right_frame = (a->flags & DSM_LRCHECK_OTHER_RIGHT_FRAME) ? 1 : 0;
  K.delt = a->delt; K.factor = a->factor; K.threshold = a->threshold;
  dsm_clear_stale_error();
  hipLaunchKernelGGL(lr_check_tiles, dim3((unsigned)(per * a->B)), dim3(256), 0, (hipStream_t)stream, K);
  return dsm_launch_status();
}

extern "C" size_t dsm_fill_background_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)B * H * sizeof(int);
}

extern "C" int dsm_fill_background(const void* disp, const void* mask, void* out, void* workspace, int B,
                                   int H, int W, dsm_stream_t stream) {
  DSM_REQUIRE(disp && mask && out && workspace, DSM_ERR_ARG);
  DSM_REQUIRE(B > 0 && H > 0 && W > 0, DSM_ERR_ARG);
  const long rows = (long)B * H;
  DSM_REQUIRE(out != disp && out != mask && out != workspace, DSM_ERR_ARG);
  if (rows < (1L << 31)) {                               // byte extents that fit: any overlap is refused too
    const size_t n = (size_t)rows * W;
    DSM_REQUIRE(!overlap(out, n * 4, disp, n * 4) && !overlap(out, n * 4, mask, n), DSM_ERR_ARG);
    DSM_REQUIRE(!overlap(workspace, (size_t)rows * 4, out, n * 4), DSM_ERR_ARG);
  }
  DSM_REQUIRE((((uintptr_t)disp | (uintptr_t)out | (uintptr_t)workspace) & 3u) == 0, DSM_ERR_ALIGN);
  DSM_REQUIRE(rows < (1L << 31), DSM_ERR_UNSUPPORTED);                        // the grid's x extent
  Fill K;
  K.disp = (const float*)disp; K.mask = (const unsigned char*)mask; K.out = (float*)out;
  K.rowflag = (int*)workspace;
  K.B = B; K.H = H; K.W = W;
  dsm_clear_stale_error();
  hipLaunchKernelGGL(fill_rows, dim3((unsigned)((long)B * H)), dim3(CH), 0, (hipStream_t)stream, K);
  hipLaunchKernelGGL(fill_empty_rows, dim3((unsigned)((long)B * H)), dim3(CH), 0, (hipStream_t)stream, K);
  return dsm_launch_status();
}
