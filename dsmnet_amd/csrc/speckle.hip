// Speckle filter of a disparity map: connected regions of the 4-neighbour graph whose edges join two
// nodes (finite, valid pixels) with fabsf(d[p] - d[q]) <= max_diff, and the removal of the regions of at
// most max_size nodes (OpenCV's filterSpeckles convention).  Beyond the reference, like lrcheck.hip;
// the semantics are in include/dsmnet_hip.h, the arguments below in DESIGN.md 20.
//
// Block-based union-find over an int32 label array in the workspace.  label[p] is the linear index
// (over B*H*W) of another node of p's region, or p itself (a root), or -1 (no node).  Four launches on
// one stream, each boundary a synchronisation:
//
//   speckle_label_tiles    one workgroup per (image, 16x64 tile), a wave per row.  The rows' runs come
//                          from a ballot (label = the run's first pixel), the rows are joined with
//                          union-find in LDS, every pixel is mapped to its tile-local root, and the
//                          nodes of each root are counted in LDS (one LDS add per (wave, root)).  Writes
//                          label[] and count[] of EVERY pixel of the tile: count = the nodes of the
//                          tile-local region at its root, 0 elsewhere.  Nothing of the workspace is read
//                          before this launch has written it.
//   speckle_merge_borders  one thread per pixel on the first column / first row of a tile (not of the
//                          image): joined to the pixel across the border if the edge exists.  The only
//                          kernel in which workgroups race on label[]: every read is a relaxed
//                          agent-scope atomic load, every write an atomicMin.  Not launched for a
//                          single-tile image.
//   speckle_flatten_count  one thread per pixel, at once done unless the pixel is a tile-local root
//                          (count > 0): its label becomes the region's root (atomicMin) and its count is
//                          added there: one integer atomicAdd per (tile, region).  The other nodes keep
//                          the label speckle_label_tiles gave them, their tile's root: unions write the
//                          labels of roots only.
//   speckle_apply          one thread per pixel: root = label[label[p]], size = count[root],
//                          keep = size > max_size, out.
//
// Invariant, from the first store on: label[x] <= x for a node, label[x] is a node of x's region, and
// label[x] only ever decreases (every write after speckle_label_tiles is an atomicMin).  Hence
//   * a find step moves to a strictly smaller index or stops: at most x steps;
//   * a stale or torn-in-time read is harmless: an older value of label[x] is still a node of the same
//     region with a smaller index, the walk merely takes another way down;
//   * a union retry continues from what atomicMin returned, strictly below the index it tried: the
//     larger of the two indices falls every pass.
// No loop waits for another thread: there is no flag, ticket or spin.  Integer min and add commute, so the
// final labels' roots (the smallest index of each region), the counts and the outputs do not depend on
// the order of execution: two runs give the same bits.
#include "common.hpp"

namespace {

constexpr int TH = 16, TW = 64, TP = TH * TW;  // tile: a wave per row, four rows per wave
static_assert(TW == DSM_WAVE, "a row of a tile is one wave: the runs come from its ballot");
static_assert(sizeof(dsm_speckle_args) == 80, "dsm_speckle_args layout (ctypes mirror in _lib.py)");

struct Work {
  const float* disp;
  const unsigned char* valid;
  float* out;
  unsigned char* keep;
  int* size;
  int* label;                                  // workspace [0, n)
  int* count;                                  // workspace [n, 2n)
  int B, H, W, nty, ntx, per;                  // per = tiles of one image
  int n;                                       // B * H * W < 2^31
  int nv, nb;                                  // border pixels of one image: vertical borders, all
  int max_size;
  float max_diff, new_val;
};

__device__ __forceinline__ bool finite_f32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// ---- LDS union-find (one workgroup; LDS is one memory, the atomic load only keeps the compiler from
// ---- holding a label in a register)
__device__ __forceinline__ int lds_load(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ int lds_find(const int* lab, int x) {
  // terminates: lab[x] <= x; every pass moves to a strictly smaller index or returns (<= x passes)
  for (;;) {
    const int p = lds_load(lab + x);
    if (p >= x || p < 0) return x;
    x = p;
  }
}

__device__ __forceinline__ void lds_unite(int* lab, int a, int b) {
  a = lds_find(lab, a);
  b = lds_find(lab, b);
  // terminates: max(a, b) strictly falls every pass (old < a when the loop goes on) and is >= 0
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(lab + a, b);     // a > b
    if (old == a) break;                       // a was a root and now hangs below b
    a = old;                                   // a had a parent old < a: unite that with b
  }
}

// ---- global union-find (speckle_merge_borders, speckle_flatten_count)
__device__ __forceinline__ int g_load(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int g_find(const int* label, int x) {
  // terminates: every pass moves to a strictly smaller index or returns (<= x passes), whatever the
  // memory holds; p < 0 cannot occur on a node's path (a node's label is a node)
  for (;;) {
    const int p = g_load(label + x);
    if (p >= x || p < 0) return x;
    x = p;
  }
}

__device__ __forceinline__ void g_unite(int* label, int a, int b) {
  a = g_find(label, a);
  b = g_find(label, b);
  // terminates: max(a, b) strictly falls every pass: the retry continues from the value atomicMin
  // returned, which is < a; nobody is waited for
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(label + a, b);
    if (old == a) break;
    a = old;
  }
}

__global__ __launch_bounds__(256) void speckle_label_tiles(const Work K) {
  __shared__ float s_d[TP];
  __shared__ int s_lab[TP];
  __shared__ int s_cnt[TP];
  __shared__ unsigned char s_node[TP];
  const int tid = threadIdx.x, wave = tid / DSM_WAVE, lane = tid % DSM_WAVE;
  const int b = blockIdx.x / K.per, local = blockIdx.x - b * K.per;
  const int y0 = (local / K.ntx) * TH, x0 = (local % K.ntx) * TW;
  const int H = K.H, W = K.W, gx = x0 + lane;
  const int base = b * (H * W);
  const float md = K.max_diff;

  bool node[4], eleft[4];
  float d[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ly = wave + 4 * k, i = ly * TW + lane, gy = y0 + ly;
    const bool inside = gy < H && gx < W;
    const int g = inside ? base + gy * W + gx : 0;
    node[k] = false;
    d[k] = 0.f;
    if (inside && (!K.valid || K.valid[g] != 0)) {       // the value of an invalid pixel is never loaded
      const float v = K.disp[g];
      if (finite_f32(v)) { node[k] = true; d[k] = v; }
    }
    s_d[i] = d[k];
    s_node[i] = node[k] ? 1 : 0;
    s_cnt[i] = 0;
    // the row's runs: joined to the left neighbour, or a run's first pixel
    const float dl = __shfl_up(d[k], 1, DSM_WAVE);
    const int nl = __shfl_up((int)node[k], 1, DSM_WAVE);
    eleft[k] = node[k] && lane > 0 && nl != 0 && fabsf(d[k] - dl) <= md;
    const unsigned long long starts = __ballot(node[k] && !eleft[k]);
    const unsigned long long below = starts & ((2ull << lane) - 1ull);      // lanes <= this one
    s_lab[i] = node[k] ? ly * TW + (63 - __clzll((long long)below)) : -1;   // a node has a start at or below it
  }
  __syncthreads();

  // join the rows.  An up edge is skipped where the left neighbour has one too and both rows run on
  // from it: that neighbour's union (or the one it relies on, down to the run's first column) covers it.
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ly = wave + 4 * k, i = ly * TW + lane;
    if (ly == 0) continue;                     // wave-uniform
    const int up = i - TW;
    const bool eu = node[k] && s_node[up] != 0 && fabsf(d[k] - s_d[up]) <= md;
    const int eu_left = __shfl_up((int)eu, 1, DSM_WAVE);
    bool covered = false;
    if (eu && lane > 0 && eleft[k] && eu_left != 0)
      covered = s_node[up - 1] != 0 && fabsf(s_d[up] - s_d[up - 1]) <= md;
    if (eu && !covered) lds_unite(s_lab, i, up);
  }
  __syncthreads();

  int root[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = (wave + 4 * k) * TW + lane;
    root[k] = node[k] ? lds_find(s_lab, i) : -1;         // nobody writes s_lab any more
    // the nodes of each root in this row: one LDS add per (wave, root)
    unsigned long long todo = __ballot(node[k]);
    while (todo) {                             // terminates: every pass clears at least the leader's bit
      const int leader = __ffsll((long long)todo) - 1;
      const int r0 = __shfl(root[k], leader, DSM_WAVE);
      const unsigned long long same = __ballot(node[k] && root[k] == r0);
      if (lane == leader) atomicAdd(s_cnt + r0, (int)__popcll(same));
      todo &= ~same;
    }
  }
  __syncthreads();

#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ly = wave + 4 * k, i = ly * TW + lane, gy = y0 + ly;
    if (gy < H && gx < W) {
      const int g = base + gy * W + gx, r = root[k];
      K.label[g] = node[k] ? base + (y0 + r / TW) * W + x0 + r % TW : -1;
      K.count[g] = (node[k] && r == i) ? s_cnt[i] : 0;
    }
  }
}

__global__ __launch_bounds__(256) void speckle_merge_borders(const Work K) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)K.B * K.nb) return;
  const int b = (int)(t / K.nb);
  int r = (int)(t - (long)b * K.nb);
  const int H = K.H, W = K.W, base = b * (H * W);
  int p, step, along;                          // q = p - step lies across the border; p - along is the
  bool first;                                  // pixel before p along it, in the same pair of tiles
  if (r < K.nv) {                              // first column of a tile: joined to the left
    const int j = r / H, y = r - j * H;
    p = base + y * W + (j + 1) * TW;
    step = 1; along = W; first = y % TH == 0;
  } else {                                     // first row of a tile: joined upwards
    r -= K.nv;
    const int j = r / W, x = r - j * W;
    p = base + (j + 1) * TH * W + x;
    step = W; along = 1; first = x % TW == 0;
  }
  const int q = p - step;
  const int lp = g_load(K.label + p), lq = g_load(K.label + q);
  if (lp < 0 || lq < 0) return;                // a label < 0 is no node, at any time
  if (!(fabsf(K.disp[p] - K.disp[q]) <= K.max_diff)) return;
  if (!first) {
    // covered by the pair before it along the border: that pair has the edge too, and p and q already
    // share a label with their predecessors (equal labels, read at any time, mean one region).  That
    // pair's thread unites it, or relies on the pair before in the same way, down to `first`.
    const int pp = p - along, pq = q - along;
    const int lpp = g_load(K.label + pp), lpq = g_load(K.label + pq);
    if (lpp >= 0 && lpq >= 0 && lpp == lp && lpq == lq && fabsf(K.disp[pp] - K.disp[pq]) <= K.max_diff) return;
  }
  g_unite(K.label, p, q);
}

__global__ __launch_bounds__(256) void speckle_flatten_count(const Work K) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= K.n) return;
  const int p = (int)t;
  // count[p] > 0: p is its tile's root of a region.  Only those have work here: the label of every other
  // node is its tile's root since speckle_label_tiles (a union writes the labels of roots only).  Adds go
  // to global roots only; a global root may read its own count half added and does nothing with it.
  const int c = g_load(K.count + p);
  if (c <= 0) return;
  // roots are not written in this kernel (atomicMin(label[r], r) changes nothing), so the root found is
  // the region's final one: its smallest index
  const int root = g_find(K.label, p);
  if (root == p) return;
  atomicMin(K.label + p, root);
  atomicAdd(K.count + root, c);
}

__global__ __launch_bounds__(256) void speckle_apply(const Work K) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= K.n) return;
  const int p = (int)t;
  const int l = K.label[p];                    // the tile's root, whose label is the region's root
  const int sz = l < 0 ? 0 : K.count[K.label[l]];        // since speckle_flatten_count
  const bool keep = sz > K.max_size;
  if (K.size) K.size[p] = sz;
  if (K.keep) K.keep[p] = keep ? 1 : 0;
  if (K.out) K.out[p] = keep ? K.disp[p] : K.new_val;    // a rejected pixel's value is not loaded
}

}  // namespace

extern "C" size_t dsm_speckle_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)B * (size_t)H * (size_t)W * 2 * sizeof(int);
}

extern "C" int dsm_speckle_filter(const dsm_speckle_args* a, dsm_stream_t stream) {
  DSM_REQUIRE(a && a->disp && a->workspace, DSM_ERR_ARG);
  DSM_REQUIRE(a->out || a->keep || a->size, DSM_ERR_ARG);
  DSM_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0, DSM_ERR_ARG);
  DSM_REQUIRE(a->max_size >= 0, DSM_ERR_ARG);
  DSM_REQUIRE(a->max_diff >= 0.f && a->max_diff <= 3.402823466e38f, DSM_ERR_ARG);   // NaN fails both
  DSM_REQUIRE(a->flags == 0, DSM_ERR_ARG);
  const uintptr_t words = (uintptr_t)a->disp | (uintptr_t)a->out | (uintptr_t)a->size | (uintptr_t)a->workspace;
  DSM_REQUIRE((words & 3u) == 0, DSM_ERR_ALIGN);
  const long rows = (long)a->B * a->H;                                               // < 2^62
  DSM_REQUIRE(rows < (1L << 31), DSM_ERR_UNSUPPORTED);                               // so that rows * W fits a long
  const long n = rows * a->W;
  DSM_REQUIRE(n < (1L << 31), DSM_ERR_UNSUPPORTED);                                  // int32 linear indices
  Work K;
  K.disp = (const float*)a->disp; K.valid = (const unsigned char*)a->valid;
  K.out = (float*)a->out; K.keep = (unsigned char*)a->keep; K.size = (int*)a->size;
  K.label = (int*)a->workspace; K.count = K.label + n;
  K.B = a->B; K.H = a->H; K.W = a->W;
  K.nty = dsm_cdiv(a->H, TH); K.ntx = dsm_cdiv(a->W, TW);
  K.per = K.nty * K.ntx;                                 // <= n / B
  K.n = (int)n;
  K.nv = (K.ntx - 1) * a->H;                             // < H * W / TW
  K.nb = K.nv + (K.nty - 1) * a->W;
  K.max_size = a->max_size; K.max_diff = a->max_diff; K.new_val = a->new_val;
  const long tiles = (long)K.per * a->B, borders = (long)K.nb * a->B;               // both < n
  const hipStream_t s = (hipStream_t)stream;
  dsm_clear_stale_error();
  hipLaunchKernelGGL(speckle_label_tiles, dim3((unsigned)tiles), dim3(256), 0, s, K);
  if (borders > 0)
    hipLaunchKernelGGL(speckle_merge_borders, dim3((unsigned)dsm_cdiv(borders, 256)), dim3(256), 0, s, K);
  hipLaunchKernelGGL(speckle_flatten_count, dim3((unsigned)dsm_cdiv(n, 256)), dim3(256), 0, s, K);
  hipLaunchKernelGGL(speckle_apply, dim3((unsigned)dsm_cdiv(n, 256)), dim3(256), 0, s, K);
  return dsm_launch_status();
}
