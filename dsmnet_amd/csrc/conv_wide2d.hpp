// Wide 3x3 2-D convolutions: Conv2d(Cin -> 256 | 512 | 1024, k3, pad 1, stride 1 | 2) + bias + ReLU of the
// DispNetC / iResNet encoders (models/dispnetcorr.py conv3b .. conv6b, models/iresnet.py conv3_1 .. conv6_1;
// models/util_conv.py conv2d_bn with bn = False), fp32 NHWC in and out, in the fp16 modes (PM = 2 "f16x2",
// PM = 1 "f16").  Included by conv_f16.hip after conv_split.hpp.
// With the window as a template argument (K = 5) also Conv2d(Cin -> 128 | 256, k5, pad 2, stride 2) + bias + ReLU:
// conv2 / conv3a of DispNet (models/dispnet.py) and the conv2 of DispNetC / iResNet -- see the note at the kernel.
//
// The regime is the opposite of the towers': small M (120 .. 7,680 output pixels per pair), large N (Cout)
// and K (9 Cin up to 9,216) -- the time is weight streaming (up to 37.7 MB of fp16 planes per layer) and
// the problem is filling 256 CUs from a GEMM with a handful of 32-row M-tiles.
//
// Work unit = (M-block, N-column, K-range):
//  * M-block: R output rows x CW columns of one image, at most 512 pixels = 16 M-tiles of 32 linearised
//    pixels, whose input box ((R-1) S + 3) x ((CW-1) S + 3) fits 768 LDS voxel slots (wide2d_geometry picks
//    R and CW on the host: the fewest rounds of M-tiles, then the fewest blocks).  The deep layers'
//    whole image (6 x 20, 12 x 40) is ONE block: the workgroup that loads a weight fragment uses it for
//    every output pixel.
//  * N-column: 64 output channels (two 32-channel blocks, waves (nw, mg) = 2 x 4), or 32 (all eight waves
//    on one block) where 64-wide columns would leave CUs without a workgroup.
//  * K-range: a contiguous range of 16-channel chunks, ksplit ranges per (M-block, N-column) so that
//    units >= CUs.  Partial sums go to the workspace [ksplit][M][Cout] as raw fp32 accumulators and a
//    second launch adds them IN INDEX ORDER, applies scale / shift / ReLU, stores y and folds max |y| --
//    no float atomics, bit-identical from run to run.  ksplit = 1: the epilogue runs here, no workspace.
//
// A workgroup (8 waves, 2 per SIMD) per chunk: the input box of the chunk is requested global -> VGPR one
// chunk ahead (buffer loads; taps outside the image are requested at an out-of-range offset and come back
// as zeros), split into fp16 planes and written to the OTHER of two LDS images
// [voxel slot][plane NP][16 ch], pitch (2 NP + 1) x 16 B -- an odd number of 16-byte units, conflict-free
// ds_read_b128 for lanes on consecutive slots; stride 2 keeps even and odd input columns of a row apart
// (row pitch XP = 2 XE) so that lanes stepping two input columns still sit on consecutive slots.  Per tap:
// one weight fragment per wave (buffer loads, ring of three -- five for the 5x5 window --, running on across
// chunks) feeds up to four
// M-tiles' product groups; each lane reads ITS pixel's fragment (the M-tiles are runs of the linearised
// block, not image rows).  One barrier per chunk.
// Weights: the packed f16 section of dsm_conv_pack_weights, [Cin/16][tap 9 | 25][Cout/32][plane 2][lane][16 B].
#pragma once

template <int PM>
struct WideCfg {
  static constexpr int NP = Prec<PM>::NP, NPW = Prec<PM>::NPW;
  static constexpr int THREADS = 512;
  static constexpr int NPF = dsmk::WIDE_SLOTS * 4 / THREADS;       // 6 staged quads per thread and chunk
  static constexpr int PITCH = 32 * NP + 16;
  static constexpr int IMG = dsmk::WIDE_SLOTS * PITCH;             // 61,440 B (f16x2) | 36,864 B (f16)
  static constexpr int LDS = 2 * IMG + 64;
  static_assert(NPF * THREADS == dsmk::WIDE_SLOTS * 4, "every slot is written every chunk");
  static_assert(LDS <= 160 * 1024, "LDS");
};

// TR: the transposed mode (plan kind 9, backward-data of the stride-2 layers).  The launch is the stride-1
// kernel over the Ho x Wo map X' with X'[2i][2j] = x[i][j] and zeros elsewhere (p.S = 1, p.Hi x p.Wi the
// extent of x itself): only the staging address differs -- a slot whose ABSOLUTE coordinate is even in both
// directions loads x[y/2][x/2], every other slot takes the out-of-range offset.
//
// K: the window (3, or 5 for plan kind 10: Conv2d(k5, pad 2, stride 2) + bias + ReLU of DispNet's conv2 / conv3a
// and the conv2 of DispNetC / iResNet).  Everything above holds with 25 taps per chunk, a box of
// ((R-1) S + 5) x ((CW-1) S + 5) voxels and the tap's column split (kx & 1, kx >> 1) over the even / odd halves
// of a row; the weights are the same section with 25 taps, [Cin/16][tap25][Cout/32][plane 2][lane][16 B].
template <int PM, bool TR = false, int K = 3>
__global__ __launch_bounds__(512, 2) void conv_wide2d_kernel(WideParams p) {
  static_assert(K == 3 || (K == 5 && !TR), "windows: 3x3, or 5x5 forward");
  constexpr int KK = K * K, PAD = (K - 1) / 2;
  using Cf = WideCfg<PM>;
  using frag = typename Prec<PM>::frag;
  constexpr int NP = Cf::NP, NPW = Cf::NPW, NPF = Cf::NPF, PITCH = Cf::PITCH, IMG = Cf::IMG;
  // the weight ring runs on across chunks, so its length divides the taps of a chunk (9 = 3 x 3, 25 = 5 x 5)
  constexpr int AHEAD = K == 5 ? 5 : 3, MT = 4;
  static_assert(KK % AHEAD == 0, "the ring's slot of a tap must not depend on the chunk");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  float* const red = reinterpret_cast<float*>(lds_raw + 2 * IMG);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int nwn = p.nwn, MG = 8 / nwn;                 // waves = nwn output blocks x MG M-tile groups
  const int nw = wave % nwn, mg = wave / nwn;
  const int NCH = p.Cin >> 4, NT = p.Cout >> 5;
  const int M = p.B * p.Ho * p.Wo;

  const SplitScale ss = split_scale<PM>(p.x_amax, p.w_amax);
  const float sx = ss.sx, so = ss.out;
  const __amdgpu_buffer_rsrc_t xrs = make_rsrc(p.x, p.xbytes), wrs = make_rsrc(p.w, p.wbytes);
  const unsigned WTAP = (unsigned)NT * NPW * 1024u;    // weight bytes per (chunk, tap)
  const unsigned WCH = (unsigned)KK * WTAP;

  int tapoff[KK];                                      // LDS bytes from a pixel's tap (0, 0) voxel
#pragma unroll
  for (int t = 0; t < KK; ++t) {
    const int ky = t / K, kx = t % K;
    tapoff[t] = (ky * p.XP + (p.S == 2 ? (kx & 1) * p.XE + (kx >> 1) : kx)) * PITCH;
  }
  const int npx = p.R * p.CW, ntile = (npx + 31) >> 5;
  const int wr_off = (tid >> 2) * PITCH + (tid & 3) * 8;       // slot (tid >> 2) + 128 k of an image
  constexpr unsigned OOBV = 0x80000000u;
  float am = 0.f;

  for (int unit = blockIdx.x; unit < p.nunits; unit += gridDim.x) {
    int u = unit;
    const int ks = u % p.ksplit; u /= p.ksplit;
    const int col = u % p.ncol; u /= p.ncol;
    const int bx = u % p.nbx; u /= p.nbx;
    const int by = u % p.nby;
    const int b = u / p.nby;
    const int y0 = by * p.R, x0 = bx * p.CW;
    const int c0 = (int)((long)ks * NCH / p.ksplit), c1 = (int)((long)(ks + 1) * NCH / p.ksplit);

    // ---- staging: slot -> input voxel, once per unit
    unsigned voff[NPF];
#pragma unroll
    for (int k = 0; k < NPF; ++k) {
      const int e = tid + k * Cf::THREADS;
      const int slot = e >> 2, q = e & 3;
      const int yy = slot / p.XP, xs = slot % p.XP;
      const int xx = p.S == 2 ? (xs < p.XE ? 2 * xs : 2 * (xs - p.XE) + 1) : xs;
      const int y = y0 * p.S - PAD + yy, x = x0 * p.S - PAD + xx;
      if constexpr (TR) {
        const bool ok = yy < p.IY && xx < p.IX && y >= 0 && x >= 0 && !((y | x) & 1) && (y >> 1) < p.Hi && (x >> 1) < p.Wi;
        voff[k] = ok ? (unsigned)(4l * ((((long)b * p.Hi + (y >> 1)) * p.Wi + (x >> 1)) * p.Cin + 4 * q)) : OOBV;
      } else {
        const bool ok = yy < p.IY && xx < p.IX && (unsigned)y < (unsigned)p.Hi && (unsigned)x < (unsigned)p.Wi;
        voff[k] = ok ? (unsigned)(4l * ((((long)b * p.Hi + y) * p.Wi + x) * p.Cin + 4 * q)) : OOBV;
      }
    }
    // ---- this wave's M-tiles mg, mg + MG, ...: each lane's pixel
    int xb[MT], opix[MT];
    bool on[MT], valid[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int tile = mg + MG * i;
      on[i] = tile < ntile;                            // wave-uniform
      const int v = 32 * tile + r;
      const int vv = min(v, npx - 1);
      const int ry = vv / p.CW, rx = vv % p.CW;
      xb[i] = ((p.S * ry) * p.XP + rx) * PITCH + h * 16;
      const int yo = y0 + ry, xo = x0 + rx;
      valid[i] = on[i] && v < npx && yo < p.Ho && xo < p.Wo;
      opix[i] = (b * p.Ho + yo) * p.Wo + xo;
    }
    f32x16 acc[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[i][j] = 0.f;

    f32x4 pf[NPF];
    auto gload = [&](int c) {
#pragma unroll
      for (int k = 0; k < NPF; ++k) pf[k] = buffer_load16(xrs, voff[k], (unsigned)c * 64u);
    };
    auto commit = [&](unsigned char* img) {
#pragma unroll
      for (int k = 0; k < NPF; ++k) {
        unsigned lo[NP], hi[NP];
        split_pair<PM>(pf[k].x, pf[k].y, sx, lo);
        split_pair<PM>(pf[k].z, pf[k].w, sx, hi);
#pragma unroll
        for (int q = 0; q < NP; ++q) {
          u32x2 v; v.x = lo[q]; v.y = hi[q];
          *reinterpret_cast<u32x2*>(img + wr_off + k * (128 * PITCH) + q * 32) = v;
        }
      }
    };
    frag wq[AHEAD][NP];
    const unsigned wlane = lane * 16u + (unsigned)(col * nwn + nw) * (NPW * 1024u);
    auto wload = [&](auto ic, int c) {
      constexpr int item = decltype(ic)::value;        // tap of chunk c
#pragma unroll
      for (int q = 0; q < NP; ++q)
        wq[item % AHEAD][q] = __builtin_bit_cast(
            frag, buffer_load16(wrs, wlane + q * 1024u, (unsigned)c * WCH + item * WTAP));
    };

    gload(c0);
    static_for<0, AHEAD - 1>([&](auto ic) { wload(ic, c0); });
    commit(lds_raw);
    __syncthreads();
    for (int c = c0; c < c1; ++c) {
      const unsigned char* const img = lds_raw + ((c - c0) & 1) * IMG;
      const bool more = c + 1 < c1;                    // uniform
      if (more) gload(c + 1);
      static_for<0, KK>([&](auto ic) {
        constexpr int item = decltype(ic)::value;
        if constexpr (item + AHEAD - 1 < KK) wload(std::integral_constant<int, item + AHEAD - 1>{}, c);
        else if (more) wload(std::integral_constant<int, item + AHEAD - 1 - KK>{}, c + 1);
        frag xq[MT][NP];
#pragma unroll
        for (int i = 0; i < MT; ++i)
          if (on[i]) {
#pragma unroll
            for (int q = 0; q < NP; ++q)
              xq[i][q] = *reinterpret_cast<const frag*>(img + xb[i] + tapoff[item] + q * 32);
          }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < MT; ++i)
          if (on[i]) mma32<PM>(acc[i], wq[item % AHEAD], xq[i]);
        __builtin_amdgcn_sched_barrier(0);
      });
      if (more) commit(lds_raw + (((c - c0) & 1) ^ 1) * IMG);
      __syncthreads();                                 // the other image is complete; this one is free
    }

    // ---- partial sums to the workspace, or (one K-range) the epilogue
    const int cbase = (col * nwn + nw) * 32 + 4 * h;
    if (p.ksplit > 1) {
#pragma unroll
      for (int i = 0; i < MT; ++i)
        if (valid[i]) {
          float* const wv = p.ws + ((long)ks * M + opix[i]) * p.Cout + cbase;
#pragma unroll
          for (int g = 0; g < 4; ++g)
            *reinterpret_cast<f32x4*>(wv + 8 * g) = f32x4{acc[i][4 * g], acc[i][4 * g + 1], acc[i][4 * g + 2], acc[i][4 * g + 3]};
        }
    } else {
      Affine af = load_affine(p.scale, p.shift, cbase);
#pragma unroll
      for (int g = 0; g < 4; ++g) af.sc[g] = af.sc[g] * so;
#pragma unroll
      for (int i = 0; i < MT; ++i)
        if (valid[i])
          store_tile<0>(acc[i], af, p.relu, p.y + (long)opix[i] * p.Cout + cbase, (const float*)nullptr, am);
    }
  }
  if (p.ksplit == 1) publish_amax<8>(p.y_amax, am, red);
}

// The K-ranges' partial sums, added in index order; scale / shift / ReLU; y and max |y|.
// One thread per four channels of a pixel.
__global__ __launch_bounds__(256) void wide2d_reduce_kernel(WideParams p) {
  __shared__ float red[4];
  const long nq = (long)p.B * p.Ho * p.Wo * (p.Cout >> 2);
  const int cq = p.Cout >> 2;
  const float so = split_scale<2>(p.x_amax, p.w_amax).out;           // the fp16 modes share it
  const f32x4* const ws = reinterpret_cast<const f32x4*>(p.ws);
  float am = 0.f;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
    f32x4 s = ws[q];
    for (int k = 1; k < p.ksplit; ++k) s += ws[k * nq + q];
    const int c = (int)(q % cq) * 4;
    const f32x4 one = {1.f, 1.f, 1.f, 1.f}, zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 sc = (p.scale ? *reinterpret_cast<const f32x4*>(p.scale + c) : one) * so;
    const f32x4 sh = p.shift ? *reinterpret_cast<const f32x4*>(p.shift + c) : zero;
    f32x4 v = s * sc + sh;
    if (p.relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
    reinterpret_cast<f32x4*>(p.y)[q] = v;
    track_amax(am, v);
  }
  publish_amax<4>(p.y_amax, am, red);
}

template <int PM, bool TR = false, int K = 3>
int launch_conv_wide2d(const WideParams& p, int grid, hipStream_t s) {
  using Cf = WideCfg<PM>;
  DSM_REQUIRE((dsm_allow_lds<conv_wide2d_kernel<PM, TR, K>>(Cf::LDS) == DSM_OK), DSM_ERR_LAUNCH);
  hipLaunchKernelGGL((conv_wide2d_kernel<PM, TR, K>), dim3((unsigned)grid), dim3(Cf::THREADS), Cf::LDS, s, p);
  if (p.ksplit > 1) {
    const long nq = (long)p.B * p.Ho * p.Wo * (p.Cout >> 2);
    const long blocks = dsm_cdiv(nq, 256);
    hipLaunchKernelGGL(wide2d_reduce_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, s, p);
  }
  return dsm_launch_status();
}
