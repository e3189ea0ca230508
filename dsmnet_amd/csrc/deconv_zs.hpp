// The z-sliding transposed convolution: ConvTranspose3d(k3, s2, p1, op1), Cin % 64 == 0 -> Cout = 32 | 64,
// fp32 tensors, on the 16-bit matrix pipe in the fp16 modes (PM = 2 "f16x2", PM = 1 "f16";
// conv_split.hpp), with the fused epilogue: folded BN, optional skip (cropped), ReLU, the output's
// absolute maximum.  Included by conv_f16.hip after conv_split.hpp and conv_zs.hpp.
//
// Replaces deconv3d_bn + skip add of models/psmnet/stackhourglass.py:35-49 (conv5, conv6 of the
// hourglasses) and GCNet's transposed layers with 64+ inputs, in place of deconv_split_kernel
// (plan kind 6, fp16 modes).  deconv_split_kernel's work item is (input tile, z-parity): output plane
// 2m reads input plane m, plane 2m + 1 reads planes m and m + 1, so every input plane was staged by
// three items; its single kind of wave queued L2 weight fragments behind HBM skip reads and output
// stores (in-order vmcnt), which are 378 of conv6's 425 MB.
//
// Structure (conv_zs.hpp's, adapted to stride 2 in every direction):
//  * z-sliding: a workgroup owns an input (TY = 2 rows x 32 columns) column -- its output is a
//    4 x 64 voxel patch of every output plane -- and walks input planes m.  Plane m is staged ONCE
//    (all channel groups) and feeds three output planes: z-tap 0 completes odd plane 2m - 1 (its
//    z-tap 2 came from plane m - 1), z-tap 1 makes even plane 2m, z-tap 2 starts odd plane 2m + 1.
//    Accumulator sets: 0 = plane 2m - 1, 1 = plane 2m, 2 = plane 2m + 1; after plane m, sets 0 and 1
//    go to the exchange buffer and set 2 becomes set 0.  Every odd plane sums its z-tap 2 (plane m)
//    before its z-tap 0 (plane m + 1), whatever the segmentation: results do not depend on the grid.
//  * equal ranges: units are (column, output-plane pair m = {2m, 2m + 1}); gridDim.x persistent
//    workgroups each take an equal range of the linearised unit space (no tail round).  A segment
//    [m0, m1) of one column stages planes m0 .. m1: plane m1 only for z-tap 0 (odd plane 2 m1 - 1);
//    where m1 = Di that plane is a virtual one of zeros -- no loads and no MFMAs, only the hand-over.
//    Z-taps whose output plane lies outside the segment are not run.
//  * Cout = 64 (conv5: 64 outputs on a small volume) is two workgroup columns of 32 channels, which
//    doubles the units and keeps conv6's accumulator and exchange sizes.  Column index = tile * NTP + nb.
//  * TWO KINDS OF WAVES (512 threads), as in conv_zs.hpp:
//      - MFMA waves (ah, xh): output channels 16 ah .. + 15 of the column's 32, input columns
//        16 xh .. + 15, both rows, all four (py, px) output classes, on 16x16x32 MFMAs.  Their only
//        vector-memory traffic is the weight ring (L2); activation fragments come from the LDS image;
//        finished planes go to the LDS exchange buffer as raw fp32.
//      - staging waves: the next chunk's activations HBM -> registers -> operand split -> LDS image
//        (DEPTH chunks in flight), and the epilogue of the planes the MFMA waves handed over a
//        chunk ago: skip values requested two chunks ahead, BN affine, ReLU, maximum, stores --
//        each wave's stores are 1 KiB contiguous (8 voxels x 32 channels).
//    One barrier per chunk.  Images are double-buffered; the exchange buffer is written once per
//    input plane (at its last channel group) and read in the following chunk, so with Cin >= 64
//    (two or more channel groups) one buffer suffices: the next write is at least two chunks later.
//  * weights: the kind-6 packed f16 section as it is ([Cin/16][tap 27][Cout/32][plane][lane][8]: the
//    32x32x16 A-operand order).  A 16x16x32 A fragment (lane (m, kg): cout m, k 8 kg .. 8 kg + 7) is
//    16 bytes of that layout: k-group c16 = 2 cg + (kg >> 1), lane 32 (kg & 1) + 16 ah + m -- a per-lane
//    offset, no reorder.  Activation unit kg of a voxel holds channels 8 kg .. 8 kg + 7 of the group.
//  * LDS: two images of 3 x 33 voxels (16 KB each in f16x2) + one exchange buffer of two output planes
//    of the patch (2 x 4 x 64 voxels x 128 B = 64 KB): 96 KB.
#pragma once


template <int PM> struct DzsCfg {
  static constexpr int NP = Prec<PM>::NP, NPW = Prec<PM>::NPW;
  static constexpr int THREADS = 512, NSTAGE = 256;   // 4 MFMA waves + 4 staging waves
  static constexpr int TY = 2, IY = TY + 1, IX = 33;  // input rows / halo box (the box's +1 row and column)
  static constexpr int NV = IY * IX;                  // 99 voxels
  static constexpr int NPF = (NV * 8 + NSTAGE - 1) / NSTAGE;       // 4 staged quads per staging thread
  static constexpr int NVP = 32 * NPF;                // units per (plane, kg) row: 128
  static constexpr int ROW = NVP * 16;                // 2,048 B (a multiple of 256: conflict-free fragment reads)
  static constexpr int IMG = NP * 4 * ROW;            // 16,384 | 8,192 B
  static constexpr int XPL = 2 * TY * 64 * 8 * 16;    // one output plane of the patch: 4 x 64 voxels x 8 quads, fp32
  static constexpr int LDS = 2 * IMG + 2 * XPL;       // two images, the exchange buffer (two planes)
  static constexpr int NSTEP = 27;                    // (pair j, z-tap) steps per chunk
#ifndef DSM_DZS_DEPTH
#define DSM_DZS_DEPTH 4
#endif
  static constexpr int DEPTH = DSM_DZS_DEPTH;         // chunks of activation loads in flight (staging waves): 2 | 4
  static_assert(DEPTH == 2 || DEPTH == 4, "the staging loop is unrolled four times");
  // weight ring: a step is TY x N terms MFMAs (6 in f16x2: ~100 cycles), so fragments are requested
  // eight steps ahead; 9 slots (9 divides NSTEP: slot = step % 9 stays consistent across chunks)
  static constexpr int WRING = 9, WAHEAD = 8;
  static_assert(NSTEP % WRING == 0 && WAHEAD < WRING, "weight ring");
  static_assert(LDS <= 160 * 1024, "LDS");
};

template <int PM>
__global__ __launch_bounds__(512, 1) void deconv_zs_kernel(ConvParams p) {
  using C = DzsCfg<PM>;
  using T = ZsTerms<PM>;
  using frag = typename Prec<PM>::frag;
  constexpr int NP = C::NP, NPW = C::NPW, TY = C::TY, IX = C::IX, NV = C::NV, NPF = C::NPF, ROW = C::ROW,
                IMG = C::IMG, XPL = C::XPL, NSTEP = C::NSTEP, WRING = C::WRING, WAHEAD = C::WAHEAD;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool staging = wave >= 4;             // wave-uniform role
  const int w4 = wave & 3;
  const int ncg = p.Cin >> 5;
  const int NTP = p.Cout >> 5;                // 32-channel workgroup columns per tile
  const int MD = (p.Do + 1) >> 1;             // output-plane pairs per column

  const int G = gridDim.x, id = blockIdx.x;
  const int logical = (G & 7) == 0 ? (id & 7) * (G >> 3) + (id >> 3) : id;   // neighbouring ranges on one XCD
  const long nunits = (long)p.ntiles * MD;
  const long u_begin = nunits * logical / G, u_end = nunits * (logical + 1) / G;
  if (u_begin >= u_end) return;

  const SplitScale ss = split_scale<PM>(p.x_amax, p.w_amax);
  const float sx = ss.sx, so = ss.out;
  unsigned char* const xch = lds_raw + 2 * IMG;
  float am = 0.f;

  // ---- chunk iterator: (input plane zi, channel group cg) of the segments of [u_begin, u_end)
  struct It { long u; int col, m0, m1, zhi, zi, cg; bool valid; };
  auto open_segment = [&](long u) {
    It q; q.u = u; q.valid = u < u_end;
    if (!q.valid) { q.col = q.m0 = q.m1 = q.zhi = q.zi = q.cg = 0; return q; }
    q.col = (int)(u / MD); q.m0 = (int)(u % MD);
    q.m1 = (int)min((long)MD, (long)q.m0 + (u_end - u));
    q.zhi = 2 * q.m1 - 1 < p.Do ? q.m1 : q.m1 - 1;   // plane m1 only for odd plane 2 m1 - 1
    q.zi = q.m0; q.cg = 0;
    return q;
  };
  auto advance = [&](It q) {
    if (++q.cg < ncg) return q;
    q.cg = 0;
    if (++q.zi <= q.zhi) return q;
    return open_segment(q.u + (q.m1 - q.m0));
  };
  // the planes a chunk hands over (its last channel group): bit 0 odd plane 2 zi - 1, bit 1 even plane 2 zi
  auto handover = [&](const It& q) {
    if (!q.valid || q.cg != ncg - 1) return 0u;
    unsigned m = 0;
    if (q.zi - 1 >= q.m0 && q.zi - 1 < q.m1 && 2 * q.zi - 1 < p.Do) m |= 1u;
    if (q.zi >= q.m0 && q.zi < q.m1) m |= 2u;
    return m;
  };

  if (staging) {
    // =====================================================================================
    // staging waves: chunk i + 1 -> image (i + 1) & 1 and the epilogue of the planes chunk i - 1
    // handed over, while the MFMA waves run chunk i
    const int stid = tid & 255;
    const unsigned vstride = (unsigned)p.Cin * 4u;
    const unsigned plane_bytes = vstride * (unsigned)p.Hi * (unsigned)p.Wi;         // < 2 GiB: checked by the host
    constexpr unsigned OOBV = 0x80000000u;
    // this thread's quads of a chunk: voxel sv + 32 k, quad sq (channels 4 sq .. + 3) -- a wave covers
    // 8 voxels x 8 quads; unit kg = sq >> 1 holds quads 2 kg (half 0) and 2 kg + 1 (half 1)
    const int sq = 2 * (lane >> 4) + (lane & 1), sv = 8 * w4 + ((lane & 15) >> 1);
    unsigned voff[NPF];
    auto column_offsets = [&](int col) {
      const int t = col / NTP;
      const int y0 = ((t / p.ntx) % p.nty) * TY, x0 = (t % p.ntx) * 32;
#pragma unroll
      for (int k = 0; k < NPF; ++k) {
        const int v = sv + 32 * k;
        const int y = y0 + v / IX, x = x0 + v % IX;
        const bool ok = v < NV && y < p.Hi && x < p.Wi;
        voff[k] = ok ? ((unsigned)y * (unsigned)p.Wi + (unsigned)x) * vstride + 16u * (unsigned)sq : OOBV;
      }
    };
    f32x4 pf[C::DEPTH][NPF];
    auto load_chunk = [&](auto setc, const It& q) {
      constexpr int set = decltype(setc)::value;
      const int b = (q.col / NTP) / (p.ntx * p.nty);
      const bool live = q.valid && q.zi < p.Di;         // plane Di: the virtual plane of zeros
      const long off = live ? ((long)b * p.Di + q.zi) * (long)plane_bytes + (long)q.cg * 128 : 0;
      const __amdgpu_buffer_rsrc_t rs = make_rsrc(reinterpret_cast<const char*>(p.x) + off, live ? plane_bytes : 0u);
#pragma unroll
      for (int k = 0; k < NPF; ++k) pf[set][k] = buffer_load16(rs, voff[k], 0);
    };
    const int st_off = (lane >> 4) * ROW + sv * 16 + (lane & 1) * 8;                 // + 512 k, + plane * 4 ROW
    auto split_chunk = [&](auto setc, unsigned char* wr) {
      constexpr int set = decltype(setc)::value;
#pragma unroll
      for (int k = 0; k < NPF; ++k) {
        unsigned lo[NP], hi[NP];
        split_pair<PM>(pf[set][k].x, pf[set][k].y, sx, lo);
        split_pair<PM>(pf[set][k].z, pf[set][k].w, sx, hi);
#pragma unroll
        for (int q = 0; q < NP; ++q) {
          u32x2 v; v.x = lo[q]; v.y = hi[q];
          *reinterpret_cast<u32x2*>(wr + q * 4 * ROW + 512 * k) = v;
        }
      }
    };
    // epilogue: this thread finishes quad qd of voxels v = (stid >> 3) + 32 k of each handed-over plane
    // (patch row v >> 6, column v & 63); the folded affine of its 4 channels in each workgroup column
    const int qd = stid & 7, ev = stid >> 3;
    f32x4 sc[2], sh[2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const int c = 32 * (nb < NTP ? nb : 0) + 4 * qd;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sc[nb][e] = p.scale ? p.scale[c + e] * so : so;
        sh[nb][e] = p.shift ? p.shift[c + e] : 0.f;
      }
    }
    struct Pend { int col, zi; unsigned m; };
    struct Where { int b, Y0, X0, nb; };
    auto where = [&](int col) {
      Where q;
      const int t = col / NTP;
      q.nb = col - t * NTP;
      q.b = t / (p.ntx * p.nty);
      q.Y0 = 2 * (((t / p.ntx) % p.nty) * TY);
      q.X0 = 2 * ((t % p.ntx) * 32);
      return q;
    };
    f32x4 resq[2][8];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int k = 0; k < 8; ++k) resq[s][k] = f32x4{0.f, 0.f, 0.f, 0.f};
    // voxel k of a plane: patch row k >> 1, column ev + 32 (k & 1); `vmask` bit k: inside the output
    auto vmask_of = [&](const Where& q) {
      unsigned m = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (q.Y0 + (k >> 1) < p.Ho && q.X0 + ev + 32 * (k & 1) < p.Wo) m |= 1u << k;
      return m;
    };
    auto load_res = [&](const Pend& e) __attribute__((always_inline)) {
      if (!e.m || !p.res) return;
      const Where q = where(e.col);
      const unsigned vm = vmask_of(q);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (!((e.m >> s) & 1u)) continue;
        const float* const rb = p.res + ((((long)q.b * p.Dr + 2 * e.zi - 1 + s) * p.Hr + q.Y0) * p.Wr + q.X0 + ev) * p.Cout +
                                32 * q.nb + 4 * qd;
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if ((vm >> k) & 1u)
            resq[s][k] = *reinterpret_cast<const f32x4*>(rb + ((k >> 1) * p.Wr + 32 * (k & 1)) * p.Cout);
      }
    };
    // ReLU as a maximum with 0 or -inf: relu 2 before the skip add, relu 1 after it
    const float lo2 = p.relu == 2 ? 0.f : -__builtin_huge_valf(), lo1 = p.relu == 1 ? 0.f : -__builtin_huge_valf();
    auto vmax = [](f32x4 v, float lo) {
      v.x = fmaxf(v.x, lo); v.y = fmaxf(v.y, lo); v.z = fmaxf(v.z, lo); v.w = fmaxf(v.w, lo);
      return v;
    };
    // all eight exchange reads of a plane first, then the arithmetic and the stores (one LDS latency per
    // plane, not one per voxel)
    auto epilogue = [&](const Pend& e) __attribute__((always_inline)) {
      if (!e.m) return;
      const Where q = where(e.col);
      const unsigned vm = vmask_of(q);
      const f32x4 s_ = q.nb ? sc[1] : sc[0], h_ = q.nb ? sh[1] : sh[0];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (!((e.m >> s) & 1u)) continue;
        f32x4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int oy = k >> 1, ox = ev + 32 * (k & 1);
          v[k] = *reinterpret_cast<const f32x4*>(xch + s * XPL + ((oy * 64 + ox) * 8 + (qd ^ ((ox >> 1) & 7))) * 16);
        }
        float* const yb = p.y + ((((long)q.b * p.Do + 2 * e.zi - 1 + s) * p.Ho + q.Y0) * p.Wo + q.X0 + ev) * p.Cout +
                          32 * q.nb + 4 * qd;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          if (!((vm >> k) & 1u)) continue;
          f32x4 o = vmax(v[k] * s_ + h_, lo2);
          if (p.res) o += resq[s][k];
          o = vmax(o, lo1);
          *reinterpret_cast<f32x4*>(yb + ((k >> 1) * p.Wo + 32 * (k & 1)) * p.Cout) = o;
          track_amax(am, o);
        }
      }
    };

    constexpr int D = C::DEPTH;
    It c0 = open_segment(u_begin);
    It lead = c0;                               // the chunk requested last
    column_offsets(c0.col);
    load_chunk(std::integral_constant<int, 0>{}, lead);
    split_chunk(std::integral_constant<int, 0>{}, lds_raw + st_off);
    static_for<1, D>([&](auto dc) {
      const It nl = advance(lead);
      if (nl.valid && nl.col != lead.col) column_offsets(nl.col);
      lead = nl;
      load_chunk(dc, lead);
    });
    It c1 = advance(c0);
    Pend pend = {0, 0, 0u};
    load_res(Pend{c0.col, c0.zi, handover(c0)});
    __syncthreads();                            // image 0 is complete
    // iteration i (P = i % 4, set P % D): c0 = chunk i (on the MFMA waves), c1 = chunk i + 1 (in set (P + 1) % D,
    // requested D - 1 iterations ago), pend = the planes chunk i - 1 handed over (their skip values in
    // resq since iteration i - 2).  Chunk i + D is requested first, into the set chunk i left; the skip
    // values of chunk i + 1's hand-over are requested last (consumed in iteration i + 2: with Cin >= 64
    // two consecutive chunks never both hand over).
    auto iteration = [&](auto pc) {
      constexpr int P = decltype(pc)::value;
      const It nl = advance(lead);
      if (nl.valid && nl.col != lead.col) column_offsets(nl.col);
      lead = nl;
      load_chunk(std::integral_constant<int, P % D>{}, lead);
      if (c1.valid) split_chunk(std::integral_constant<int, (P + 1) % D>{}, lds_raw + ((P + 1) & 1) * IMG + st_off);
      epilogue(pend);
      pend = Pend{c0.col, c0.zi, handover(c0)};
      load_res(Pend{c1.col, c1.zi, handover(c1)});
      __syncthreads();                          // chunk i done: image (i + 1) & 1 complete, its hand-over written
      c0 = c1; c1 = advance(c1);
      return !c0.valid;
    };
    while (true) {
      if (iteration(std::integral_constant<int, 0>{})) break;
      if (iteration(std::integral_constant<int, 1>{})) break;
      if (iteration(std::integral_constant<int, 2>{})) break;
      if (iteration(std::integral_constant<int, 3>{})) break;
    }
    epilogue(pend);
  } else {
    // =====================================================================================
    // MFMA waves
    const int j = lane & 15, kg = lane >> 4;
    const int ah = w4 >> 1, xh = w4 & 1;
    const unsigned tstride = (unsigned)NTP * (NPW * 1024);                 // bytes per tap of a k-group
    const __amdgpu_buffer_rsrc_t wrsrc = make_rsrc(p.w, p.wbytes);
    const unsigned wlane = (unsigned)(kg >> 1) * 27u * tstride + (unsigned)(32 * (kg & 1) + 16 * ah + j) * 16u;
    auto wbase_of = [&](const It& q) {
      return (unsigned)q.cg * 54u * tstride + (unsigned)(q.col % NTP) * (NPW * 1024);
    };
    const int rd_off = kg * ROW + (16 * xh + j) * 16;
    f32x4 acc[3][4][TY];                        // [z-tap set][class 2 py + px][row]
    frag xq[2][TY][NP];                         // activation fragments of input offset o, o + 1
    frag wq[WRING][NP];
    auto zero_set = [&](auto sc_) {
      constexpr int s = decltype(sc_)::value;
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < TY; ++r) acc[s][c][r] = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    // step s = 3 j + kz: pair j (dc_pair: input offset o, class c), z-tap kz
    auto wload = [&](auto sc_, unsigned wb) {
      constexpr int s = decltype(sc_)::value;
      constexpr int tap = (s % 3) * 9 + dc_tap9(s / 3);
#pragma unroll
      for (int q = 0; q < NP; ++q)
        wq[s % WRING][q] = __builtin_bit_cast(frag, buffer_load16(wrsrc, wlane, wb + (unsigned)tap * tstride + q * 1024));
    };
    auto xload = [&](auto oc, const unsigned char* rd) {
      constexpr int o = decltype(oc)::value, iy = o >> 1, ix = o & 1;
#pragma unroll
      for (int r = 0; r < TY; ++r)
#pragma unroll
        for (int q = 0; q < NP; ++q)
          xq[o & 1][r][q] = *reinterpret_cast<const frag*>(rd + q * 4 * ROW + ((r + iy) * IX + ix) * 16);
    };
    // z-taps to run on plane zi: kz 1 / 2 feed planes 2 zi / 2 zi + 1 (pair zi), kz 0 plane 2 zi - 1 (pair zi - 1)
    auto zmask_of = [&](const It& q) {
      unsigned m = 0;
      if (q.zi >= q.m0 && q.zi < q.m1) m |= 6u;
      if (q.zi - 1 >= q.m0 && q.zi - 1 < q.m1 && q.zi < p.Di && 2 * q.zi - 1 < p.Do) m |= 1u;
      return m;
    };
    It cur = open_segment(u_begin);
    static_for<0, 3>([&](auto s) { zero_set(s); });
    static_for<0, WAHEAD>([&](auto sc_) { wload(sc_, wbase_of(cur)); });
    int i = 0;
    __syncthreads();                            // image 0 is complete
    while (true) {
      const unsigned char* const rd = lds_raw + (i & 1) * IMG + rd_off;
      const It nxt = advance(cur);
      const unsigned wcur = wbase_of(cur);
      const unsigned wnext = nxt.valid ? wbase_of(nxt) : 0u;
      const unsigned mask = zmask_of(cur);
      xload(std::integral_constant<int, 0>{}, rd);
      __builtin_amdgcn_sched_barrier(0);
      static_for<0, NSTEP>([&](auto sc_) {
        constexpr int s = decltype(sc_)::value;
        constexpr int jp = s / 3, kz = s % 3;
        constexpr DcPair pr = dc_pair(jp);
        constexpr bool fresh = kz == 0 && (jp == 0 || jp == 4 || jp == 6 || jp == 8);
        if constexpr (s + WAHEAD < NSTEP) wload(std::integral_constant<int, s + WAHEAD>{}, wcur);
        else wload(std::integral_constant<int, s + WAHEAD - NSTEP>{}, wnext);
        if constexpr (fresh && pr.o + 1 < 4) xload(std::integral_constant<int, pr.o + 1>{}, rd);
        __builtin_amdgcn_sched_barrier(0);
        if ((mask >> kz) & 1u) {
          static_for<0, T::N>([&](auto tc) {
            constexpr int t = decltype(tc)::value;
            static_for<0, TY>([&](auto rc) {
              constexpr int r = decltype(rc)::value;
              acc[kz][pr.c][r] = zs_mfma<PM>(wq[s % WRING][T::w[t]], xq[pr.o & 1][r][T::x[t]], acc[kz][pr.c][r]);
            });
          });
        }
        __builtin_amdgcn_sched_barrier(0);
      });
      if (cur.cg == ncg - 1) {                  // plane zi done: hand planes 2 zi - 1 and 2 zi over, rotate
        const unsigned m = handover(cur);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          if (!((m >> s) & 1u)) continue;
#pragma unroll
          for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < TY; ++r) {
              const int oy = 2 * r + (c >> 1), ox = 2 * (16 * xh + j) + (c & 1);
              const int unit = (oy * 64 + ox) * 8 + ((4 * ah + kg) ^ (j & 7));
              *reinterpret_cast<f32x4*>(xch + s * XPL + unit * 16) = acc[s][c][r];
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int r = 0; r < TY; ++r) acc[0][c][r] = acc[2][c][r];
        zero_set(std::integral_constant<int, 1>{});
        zero_set(std::integral_constant<int, 2>{});
      }
      __syncthreads();                          // chunk i done
      cur = nxt; ++i;
      if (!cur.valid) break;
    }
  }
  // ---- the tensor maximum: one atomic per workgroup
  publish_amax<8>(p.y_amax, am, reinterpret_cast<float*>(lds_raw));
}

template <int PM>
int run_deconv_zs(ConvParams p, hipStream_t s) {
  using C = DzsCfg<PM>;
  DSM_REQUIRE(p.Cin % 64 == 0 && (p.Cout == 32 || p.Cout == 64) && 4l * p.Hi * p.Wi * p.Cin < 0x7fffffffl,
              DSM_ERR_UNSUPPORTED);       // make_plan's test (Plan::zs)
  p.ntx = dsm_cdiv(p.Wi, 32); p.nty = dsm_cdiv(p.Hi, C::TY);
  const long ncol = (long)p.B * p.nty * p.ntx * (p.Cout / 32);
  DSM_REQUIRE(ncol * p.Di < (1L << 30), DSM_ERR_UNSUPPORTED);
  p.ntiles = (int)ncol;
  const long nunits = ncol * ((p.Do + 1) / 2);
  DSM_REQUIRE(dsm_allow_lds<deconv_zs_kernel<PM>>(C::LDS) == DSM_OK, DSM_ERR_LAUNCH);
  int blocks = p.force_blocks ? p.force_blocks : 256;          // persistent workgroups: one per CU
  if ((long)blocks > nunits) blocks = (int)nunits;
  hipLaunchKernelGGL(deconv_zs_kernel<PM>, dim3(blocks), dim3(C::THREADS), C::LDS, s, p);
  return dsm_launch_status();
}
