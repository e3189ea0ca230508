// Shared pieces of the convolution translation units (conv3d.hip: fp32-input MFMA + bf16x3
// kernels; conv_f16.hip: the fp16 split kernels): tile walk, epilogue, buffer loads, launch helper.
#pragma once
#include "split_core.hpp"    // static_for, Prec / split_pair / mma32, the exponent rule, track_amax / publish_amax

namespace dsmk {

struct ConvParams {
  const float* x; const float* w; const float* scale; const float* shift;
  const float* res; float* y;
  int force_blocks;           // 0, or the persistent grid size asked for in dsm_conv3d_args.flags
  int single_kind;            // dsm_conv3d_args.flags & DSM_CONV_NO_ONCE: the chunk-pipelined single-kind kernels (A/B runs)
  int B, Cin, Cout;
  int Di, Hi, Wi, Do, Ho, Wo, Dr, Hr, Wr;
  int relu;
  int ntx, nty, ntiles;       // tile grid: x tiles, y tiles, total = B*Do*nty*ntx (x8 classes for deconv)
  unsigned xbytes, wbytes;    // extents of x and w for the buffer descriptors (< 4 GiB)
  int ntp;                    // Cout / 32 of the layer (packing and output stride); a launch may
                              // compute only NT of them per workgroup column (blockIdx.y: N-split)
  // fp16 split kernels (conv_split.hpp, PM < 3): absolute maxima of the input tensor (device scalar
  // written by its producer) and of the weights (header of the packed f16 section)
  const float* x_amax; const float* w_amax;
  float* y_amax;              // or null: max |y| of this launch is folded in (atomic max of the float bits)
};

// One place decides the kernel variant; dsm_conv3d_fwd launches it, dsm_conv3d_plan names it.  (DESIGN.md and
// the tests call the kinds by number: "kind 8".)
enum Kind : int {
  KIND_CONV = 0,           // fp32-input MFMA convolution
  KIND_DECONV = 1,         // ... transposed
  KIND_COUT1 = 2,          // conv cout1
  KIND_DECONV_COUT1 = 3,   // deconv cout1
  KIND_COUT1_ZS = 4,       // conv cout1 z-sliding
  KIND_SPLIT = 5,          // conv split (bf16x3 / f16x2 / f16)
  KIND_DECONV_SPLIT = 6,   // deconv split
  KIND_ZS = 7,             // z-sliding conv (Cout = 32, stride 1; conv_zs.hpp)
  KIND_WIDE = 8,           // wide 2-D conv (Cout 256 / 512 / 1024; conv_wide2d.hpp)
  KIND_WIDE_TR = 9,        // its transposed mode (stride 2; backward-data of the stride-2 wide layers)
  KIND_K5 = 10,            // the 5x5 stride-2 2-D conv (Cout 128 / 256; conv_wide2d.hpp with K = 5, fp16 modes only)
};
constexpr bool kind_is_wide(Kind k) { return k == KIND_WIDE || k == KIND_WIDE_TR || k == KIND_K5; }
constexpr bool kind_scales_operands(Kind k) { return k >= KIND_SPLIT; }      // reads x_amax in the fp16 modes
constexpr bool kind_bounds_own_extents(Kind k) { return k >= KIND_ZS; }      // the others: make_plan's 4 GiB bound
// zs (KIND_DECONV_SPLIT, fp16 modes): the z-sliding transposed convolution (deconv_zs.hpp) instead of deconv_split_kernel
struct Plan { Kind kind; int S, NT, TM, CK; int KZ, K, DIL; int nsplit = 1; int pm = 3; int once = 0; int zs = 0; };

// The compiled variants of the kernels that exist in several instantiations.  Each list is expanded twice:
// into plan_compiled() below, which make_plan consults, and into the chain of launches of its kind
// (launch_mfma for KIND_CONV / KIND_DECONV, dispatch_split for KIND_SPLIT) -- a plan that make_plan returns therefore
// launches, and a variant missing here is DSM_ERR_UNSUPPORTED from the plan query and the launch alike.
// KIND_CONV, 2-D (KZ = 1; 16-channel chunks): (S, NT, TM, K, DIL)
#define DSM_CONV2D_VARIANTS(X) \
  X(1, 1, 1, 3, 1) X(1, 1, 2, 3, 1) X(1, 2, 1, 3, 1) X(1, 4, 1, 3, 1) X(1, 4, 1, 3, 2) \
  X(2, 1, 1, 3, 1) X(2, 2, 1, 3, 1) X(1, 1, 1, 1, 1) X(1, 4, 1, 1, 1) X(2, 2, 1, 1, 1)
// KIND_CONV, 3-D: (S, NT, TM, CK); the N-split forms (nsplit > 1) are the NT = 1, TM = 1 variants
#define DSM_CONV3D_VARIANTS(X) \
  X(1, 1, 2, 16) X(1, 1, 1, 16) X(1, 2, 2, 8) X(1, 2, 1, 16) X(1, 4, 1, 16) X(2, 1, 1, 8) X(2, 2, 1, 8) X(2, 4, 1, 8)
// KIND_DECONV: (NT, CK)
#define DSM_DECONV3D_VARIANTS(X) X(1, 16) X(2, 16)
// KIND_SPLIT at stride 1, every precision mode: (NT, TM, KZ, DIL, NSPLIT).  (Stride 2 is <NT=2,TM=1> alone; the
// single-tile `once` form is <1, 2, 1, 1, 2> with 64 inputs in the fp16 modes.)
#define DSM_SPLIT_VARIANTS(X) \
  X(1, 4, 3, 1, 1) X(1, 2, 3, 1, 1) X(2, 2, 3, 1, 1) X(2, 1, 3, 1, 1) \
  X(1, 4, 1, 1, 1) X(1, 2, 1, 1, 1) X(2, 2, 1, 1, 1) X(2, 1, 1, 1, 1) X(4, 2, 1, 1, 1) X(4, 2, 1, 2, 1) \
  X(1, 2, 1, 1, 2) X(2, 2, 1, 1, 2) X(1, 1, 3, 1, 2) X(1, 1, 3, 1, 4)

// Is the kernel variant that `pl` selects compiled?  (The kinds without a case are single kernels.)
inline bool plan_compiled(const Plan& pl) {
  switch (pl.kind) {
    case KIND_CONV:
      if (pl.KZ == 1) {
        if (pl.nsplit != 1 || pl.CK != 16) return false;
#define DSM_X(S_, NT_, TM_, K_, DIL_) \
        if (pl.S == S_ && pl.NT == NT_ && pl.TM == TM_ && pl.K == K_ && pl.DIL == DIL_) return true;
        DSM_CONV2D_VARIANTS(DSM_X)
#undef DSM_X
        return false;
      }
      if (pl.nsplit != 1 && !(pl.NT == 1 && pl.TM == 1)) return false;
#define DSM_X(S_, NT_, TM_, CK_) if (pl.S == S_ && pl.NT == NT_ && pl.TM == TM_ && pl.CK == CK_) return true;
      DSM_CONV3D_VARIANTS(DSM_X)
#undef DSM_X
      return false;
    case KIND_DECONV:
#define DSM_X(NT_, CK_) if (pl.S == 2 && pl.NT == NT_ && pl.TM == 1 && pl.CK == CK_) return true;
      DSM_DECONV3D_VARIANTS(DSM_X)
#undef DSM_X
      return false;
    case KIND_SPLIT:
      // the stride-2, `once` and KIND_DECONV_SPLIT forms are no list: these three lines and the head of dispatch_split
      // (conv_split.hpp) are written by hand and must say the same (`once` is set from Cin == 64 only, which
      // the launch checks again); the name table of tests/test_conv_plans.py holds both to the launch
      if (pl.S == 2) return pl.NT == 2 && pl.TM == 1 && pl.KZ == 3 && pl.DIL == 1 && pl.nsplit == 1;
      if (pl.once && !(pl.NT == 1 && pl.TM == 2 && pl.KZ == 1 && pl.DIL == 1 && pl.nsplit == 2)) return false;
#define DSM_X(NT_, TM_, KZ_, DIL_, NSPLIT_) \
      if (pl.NT == NT_ && pl.TM == TM_ && pl.KZ == KZ_ && pl.DIL == DIL_ && pl.nsplit == NSPLIT_) return true;
      DSM_SPLIT_VARIANTS(DSM_X)
#undef DSM_X
      return false;
    case KIND_DECONV_SPLIT: return pl.NT == 1 || pl.NT == 2;
    default: return true;
  }
}

#ifndef DSM_DECONV_ZS
#define DSM_DECONV_ZS 1       // 0: plan kind 6 stays on deconv_split_kernel in the fp16 modes (A/B builds)
#endif

// the z-sliding kernel (conv_zs.hpp, plan kind 7)
struct ZsParams {
  const float* x;               // fp32 NDHWC (B,Di,Hi,Wi,Cin), or (vol) the NHWC features (2B,Hi,Wi,Cin/2)
  const unsigned char* w;       // packed by pack_weights_zs_kernel<PM> (past the header)
  const float* scale; const float* shift;
  const float* res;             // fp32 NDHWC (B,Dr,Hr,Wr,32) or null
  float* y;                     // fp32 NDHWC (B,Do,Ho,Wo,32)
  const float* x_amax; const float* w_amax; float* y_amax;
  int B, Cin;
  int Di, Hi, Wi, Do, Ho, Wo, Dr, Hr, Wr;
  int relu;
  int vol, vol_mask_left;
  int ntx, nty, ncol;           // columns: (b, ty, tx), 8 x 32 outputs each
  long nunits;                  // ncol * Do
  unsigned wbytes;
};

// conv_f16.hip: the fp16 kernels (plan kinds 5 / 6 / 7 with pm = 2 | 1)
__attribute__((visibility("hidden"))) int run_split_f16(const Plan& pl, const ConvParams& p, hipStream_t s);
__attribute__((visibility("hidden"))) int run_zs_f16(int pm, const ZsParams& p, int grid, hipStream_t s);

// the fused 64-channel BasicBlock (basicblock2d.hpp)
struct BbParams {
  const float* x; float* y;
  const unsigned char* w1; const unsigned char* w2;       // fp16 planes [Cin/16][tap9][n 2][plane][lane][16 B]
  const float* w1_amax; const float* w2_amax;
  const float* scale1; const float* shift1; const float* scale2; const float* shift2;
  const float* x_amax; float* y_amax;
  int B, H, W, C, relu, skip, ntx, nty, ntiles;           // relu: 1 = ReLU at the end (GCNet's block); skip: 1 = + x
  unsigned xbytes, wbytes;
};

__attribute__((visibility("hidden"))) int run_basicblock_f16(int pm, const BbParams& p, hipStream_t s);

// the wide 2-D convolution (conv_wide2d.hpp, plan kind 8): Cout = 256 | 512 | 1024, fp16 modes; with a 5x5
// window at stride 2 (plan kind 10): Cout = 128 | 256
constexpr int WIDE_SLOTS = 768;     // LDS voxel slots of one staged input box
constexpr int WIDE_PIXELS = 512;    // output pixels of an M-block: 8 waves x 4 M-tiles of 32 / 2 output blocks
struct WideParams {
  const float* x;
  const unsigned char* w;       // the packed f16 section past its header
  const float* scale; const float* shift;
  float* y;
  float* ws;                    // [ksplit][B*Ho*Wo][Cout] partial sums (ksplit > 1)
  const float* x_amax; const float* w_amax; float* y_amax;
  int B, Cin, Cout, Hi, Wi, Ho, Wo, S, relu;     // kind 9: S = 1 over Ho x Wo, Hi x Wi the extent of x itself
  int R, CW, nby, nbx;          // M-block: R output rows x CW columns; blocks per image
  int IY, IX, XP, XE;           // input box rows / columns, LDS row pitch in slots, even-column count (S = 2)
  int nwn, ncol;                // 32-channel output blocks per workgroup (2 | 1), N-columns = Cout / (32 nwn)
  int ksplit, nunits;
  unsigned xbytes, wbytes;
  int K = 3;                    // window (host side: the geometry; the kernel has it as a template argument)
};
// M-block of a layer: the (R, CW) with the fewest rounds of M-tiles (a round = one M-tile on each of four
// wave groups), then the fewest blocks, among column splits nbx = 1 .. 8.  False: no block fits.
// The box of a block is ((R-1) S + K) x ((CW-1) S + K) voxels for a K x K window.
inline bool wide2d_geometry(WideParams& p) {
  long best = -1;
  for (int nbx = 1; nbx <= 8; ++nbx) {
    const int CW = (p.Wo + nbx - 1) / nbx;
    const int IX = (CW - 1) * p.S + p.K, XE = (IX + 1) / 2, XP = p.S == 1 ? IX : 2 * XE;
    if (CW > WIDE_PIXELS || p.K * XP > WIDE_SLOTS) continue;
    int R = WIDE_PIXELS / CW;
    const int rl = (WIDE_SLOTS / XP - p.K) / p.S + 1;
    if (rl < R) R = rl;
    if (p.Ho < R) R = p.Ho;
    const int nby = (p.Ho + R - 1) / R;
    R = (p.Ho + nby - 1) / nby;
    const int tiles = (R * CW + 31) / 32;
    const long cost = (long)nbx * nby * ((tiles + 3) / 4) * 1024 + nbx * nby;
    if (best < 0 || cost < best) {
      best = cost;
      p.R = R; p.CW = CW; p.nbx = nbx; p.nby = nby;
      p.IY = (R - 1) * p.S + p.K; p.IX = IX; p.XP = XP; p.XE = XE;
    }
  }
  return best >= 0;
}
__attribute__((visibility("hidden"))) int run_wide2d_f16(int pm, const WideParams& p, int grid, int transposed, hipStream_t s);

}  // namespace dsmk

namespace {

using namespace dsmk;      // the structs, Kind and its enumerators, the run_* entry points

constexpr int NTHREADS = 256;

// Input-tile geometry for an output tile of TY rows x 32 columns, one z.
// KZ x KXY x KXY taps (KZ = 1: a 2-D convolution on (B,1,H,W,C) volumes), dilation DIL in
// (y, x), padding = "same" ((K-1)/2 * dilation), stride S.
template <int S, int KZ = 3, int KXY = 3, int DIL = 1> struct Geo {
  static constexpr int IZ = KZ;
  static constexpr int EXT = (KXY - 1) * DIL;           // halo span in y and x
  static constexpr int PADZ = (KZ - 1) / 2, PADXY = EXT / 2;
  static constexpr int NTAP = KZ * KXY * KXY;
  static __host__ __device__ constexpr int IY(int TY) { return (TY - 1) * S + EXT + 1; }
  static constexpr int IX = 31 * S + EXT + 1;           // 34 or 65 for the 3x3x3 trunk
  static constexpr int XE = (IX + 1) / 2;               // even columns when S == 2
  static constexpr int XP = (S == 1) ? IX : 2 * XE;     // LDS row pitch in 16-B elements
  static __host__ __device__ constexpr int xmap(int x) {
    return S == 1 ? x : ((x & 1) * XE + (x >> 1));
  }
};

// XCD-aware persistent tile order: workgroups are dealt round-robin over the 8
// XCDs, so worker (xcd = id % 8, slot = id / 8) walks a contiguous eighth of the
// tile space -- neighbouring tiles (shared halos) meet in one XCD's L2.  Speed only.
__device__ __forceinline__ int first_tile(int ntiles, int& step, int& end) {
  const int id = blockIdx.x, G = gridDim.x;
  if ((G & 7) != 0 || ntiles < 64) { step = G; end = ntiles; return id; }
  const int xcd = id & 7, slot = id >> 3;
  const int per = (ntiles + 7) >> 3;
  const int lo = xcd * per;
  end = min(ntiles, lo + per);
  step = G >> 3;
  return lo + slot;
}

// Epilogue of one 32x32 accumulator tile.  The MFMAs are issued with the WEIGHT fragment as
// the A operand and the activation fragment as B, so the tile comes out transposed: lane
// (r = lane & 31, h = lane >> 5) owns output voxel r of the row and register k holds channel
// (k & 3) + 8 (k >> 2) + 4 h -- four consecutive channels per register quad, i.e. 16
// contiguous bytes of the NDHWC voxel.  Each lane therefore issues 4 dwordx4 stores (and 4
// dwordx4 skip loads) per tile instead of 16 dword ones: the store tail is issue-bound, not
// bandwidth-bound (measured: ~20k cycles per tile with dword stores).
//   y = acc*scale + shift (ReLU?) (+ skip) (ReLU?)
// `yv` / `rv` point at this lane's voxel, channel 32*n + 4*h; XS = voxel stride between
// consecutive lanes (1, or 2 for a transposed-conv parity class).
// per-lane epilogue constants: scale/shift of the 16 channels this lane owns in one N-tile
struct Affine { f32x4 sc[4], sh[4]; };
__device__ __forceinline__ Affine load_affine(const float* __restrict__ scale,
                                              const float* __restrict__ shift, int cbase) {
  Affine a;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const f32x4 one = {1.f, 1.f, 1.f, 1.f}, zero = {0.f, 0.f, 0.f, 0.f};
    a.sc[g] = scale ? *reinterpret_cast<const f32x4*>(scale + cbase + 8 * g) : one;
    a.sh[g] = shift ? *reinterpret_cast<const f32x4*>(shift + cbase + 8 * g) : zero;
  }
  return a;
}

// The epilogue of one 32-voxel x 32-channel accumulator tile, in two halves: `load_residual` requests the
// skip tensor's values, `store_tile` finishes and stores.  A kernel with several tiles per epilogue
// (rows, output blocks, the four classes of the transposed convolution) calls load_residual for ALL
// of them first: left to one call per tile, the next tile's loads cannot move above the previous
// tile's stores (they may alias as far as the compiler knows), and every tile exposes a full memory
// latency -- the transposed 64 -> 32 kernel spent most of its 170 us there (profiles/r03_ablation.md, 5).
struct Residual { f32x4 v[4]; };
__device__ __forceinline__ void load_residual(Residual& r, const float* __restrict__ rv) {
#pragma unroll
  for (int g = 0; g < 4; ++g) r.v[g] = *reinterpret_cast<const f32x4*>(rv + 8 * g);
}
template <int COUT>
__device__ __forceinline__ void store_tile(const f32x16& acc, const Affine& af, int relu,
                                           float* __restrict__ yv, const Residual& res, bool has_res, float& am) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const f32x4 sc = af.sc[g], sh = af.sh[g];
    f32x4 v = {acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
    v = v * sc + sh;
    if (relu == 2) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
    if (has_res) v += res.v[g];
    if (relu == 1) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
    *reinterpret_cast<f32x4*>(yv + 8 * g) = v;
    track_amax(am, v);
  }
}
// one tile, residual requested and consumed on the spot (the fp32-input kernels, single-tile epilogues)
template <int COUT>
__device__ __forceinline__ void store_tile(const f32x16& acc, const Affine& af, int relu,
                                           float* __restrict__ yv, const float* __restrict__ rv, float& am) {
  Residual r;
#pragma unroll
  for (int g = 0; g < 4; ++g) r.v[g] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (rv) load_residual(r, rv);
  store_tile<COUT>(acc, af, relu, yv, r, rv != nullptr, am);
}

// ----------------------------------------------------------------------------
// Staging of one channel chunk of a halo tile: global -> registers -> LDS.
//
// On gfx950 the fp32 MFMA shares the SIMD's vector ALU ("runs at the vector rate"): every
// VALU instruction of either resident wave is time taken from the matrix pipe (stamps: two
// workgroups per CU spend 2 x 27.6k cycles in MFMAs + 2 x 6.6k in VALU per pair of chunks,
// and staging code that runs 3k cycles alone takes 14k beside a multiplying partner).  So
// the staging path is built to issue (almost) no VALU:
//  * the LDS image is stored in element order e = ((z*IY + y)*IX + x)*NQ + q and thread
//    `tid` owns elements e = tid + 256*k: a commit is NPF ds_write_b128 with immediate
//    offsets (the A-fragment reads then have a 4-way bank conflict, irrelevant beside
//    64-cycle MFMAs);
//  * each thread's global offsets are computed once per launch; a chunk whose halo box lies
//    inside the volume (wave-uniform test) is staged by loads of the form
//    scalar base + 32-bit register offset, zero VALU; boxes that stick out of the volume
//    (edge tiles) take a guarded path that decodes coordinates on the fly;
//  * the loads are issued one per item inside the multiply loop.
// ----------------------------------------------------------------------------
// 16-byte load through a buffer descriptor: address = descriptor base + voffset (VGPR, fixed per
// lane) + soffset (SGPR).  No address VALU at all, which is the point here (T8 in the guide).
__device__ __forceinline__ f32x4 buffer_load16(__amdgpu_buffer_rsrc_t rsrc, unsigned voffset,
                                               unsigned soffset) {
  const auto v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)voffset, (int)soffset, 0);
  static_assert(sizeof(v) == 16, "raw_buffer_load_b128 must return 16 bytes");
  return __builtin_bit_cast(f32x4, v);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}



template <auto kernel>
int launch_tiles(const ConvParams& p, size_t lds, hipStream_t s, int max_blocks, int ny = 1) {
  if (lds > 64 * 1024 && dsm_allow_lds<kernel>(lds) != DSM_OK) return DSM_ERR_LAUNCH;
  if (p.force_blocks) max_blocks = p.force_blocks;     // dsm_conv3d_args.flags: persistent-grid A/B runs
  int blocks = p.ntiles < max_blocks ? p.ntiles : max_blocks;
  if (blocks >= 8) blocks &= ~7;                 // whole rounds over the 8 XCDs
  hipLaunchKernelGGL(kernel, dim3(blocks, ny), dim3(NTHREADS), lds, s, p);
  return dsm_launch_status();
}

}  // namespace
