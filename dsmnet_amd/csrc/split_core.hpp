// The precision core of the 16-bit matrix-pipe kernels and the tensor-maximum slots that
// feed it: the ONE definition of the operand split, the MFMA term order, the power-of-two
// exponent rule, the launch scale and the max |y| publishers.  Forward kernels (conv_split.hpp, conv_zs.hpp,
// deconv_zs.hpp, conv_wide2d.hpp, basicblock2d.hpp), the weight gradient (conv3d_bwd.hip) and the
// element-wise producers of a slot (bn3d.hip, spp.hip, sepvol.hip, relu_bwd.hip) all take them from here.
//
// PM (precision mode) = number of 16-bit terms an fp32 operand is split into:
//   PM = 3  "bf16x3": v = hi + mid + lo in bf16 (exact split), six MFMAs per product -- fp32 accuracy,
//           no scaling needed (bf16 has the fp32 exponent range);
//   PM = 2  "f16x2":  v * 2^e = hi + lo in fp16 (22 significand bits), three MFMAs per product
//           (wl xh + wh xl + wh xh) -- fp32 accuracy at half the MFMAs.  fp16 has a 5-bit exponent,
//           so every tensor is scaled by a power of two chosen from its absolute maximum (activations:
//           a device scalar written by the producing kernel's epilogue, dsm_conv3d_args.x_amax /
//           y_amax; weights: at pack time) so that the maximum lands in [2^12, 2^13); the combined
//           2^-(ex + ew) is folded into the epilogue's scale.  Residuals that fall below fp16's normal
//           range become subnormals (absolute error 2^-25 against a maximum of 2^12), which the MFMA
//           keeps (f16 denormals are not flushed on gfx950: tests/test_f16_gpu.py);
//   PM = 1  "f16":    operands rounded to fp16 (hi only), one MFMA per product, fp32 accumulate --
//           the reduced-precision mode of BASELINE config #5.
#pragma once
#include "common.hpp"
#include <type_traits>

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// Compile-time loop: f(integral_constant<int, I>) for I in [I0, N).  Used where an index must
// be a constant expression so that accumulator arrays stay in registers (a runtime-indexed
// ext-vector array goes to scratch).
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

template <int PM> struct Prec;
template <> struct Prec<3> { static constexpr int NP = 3, NPW = 3; typedef bf16x8 frag; };
template <> struct Prec<2> { static constexpr int NP = 2, NPW = 2; typedef f16x8 frag; };
template <> struct Prec<1> { static constexpr int NP = 1, NPW = 2; typedef f16x8 frag; };   // reads plane 0 of the f16x2 packing

__device__ __forceinline__ unsigned pack_bf16(float a, float b) {        // low half = a
  const f32x2 t = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(t, bf16x2));
}
__device__ __forceinline__ float bf16_lo(unsigned u) { return __builtin_bit_cast(float, u << 16); }
__device__ __forceinline__ float bf16_hi(unsigned u) { return __builtin_bit_cast(float, u & 0xffff0000u); }

// two fp32 values -> their NP planes (one dword per plane, low half = a).  PM < 3: `sx` = 2^ex.
template <int PM>
__device__ __forceinline__ void split_pair(float a, float b, float sx, unsigned (&pl)[Prec<PM>::NP]) {
  if constexpr (PM == 3) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      pl[q] = pack_bf16(a, b);
      if (q < 2) { a -= bf16_lo(pl[q]); b -= bf16_hi(pl[q]); }
    }
  } else {
    // hi = f16(v * sx) straight from the fp32 value (v_fma_mix{lo,hi}_f16: an fp32 fma -- exact, sx is a
    // power of two -- rounded once to fp16), the residual with hi read as an fp16 operand
    // (v_fma_mix_f32): five plain VALU instructions per pair and no packed-fp32 ones, which issue
    // slowly beside an MFMA stream (MI355X_MICROARCH.md, "price of one filler beside MFMAs")
    unsigned hi;
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(hi) : "v"(a), "s"(sx));
    asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(hi) : "v"(b), "s"(sx));
    pl[0] = hi;
    if constexpr (PM == 2) {
      float r0, r1;
      asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(r0) : "v"(a), "s"(sx), "v"(hi));
      asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(r1) : "v"(b), "s"(sx), "v"(hi));
      const f32x2 r = {r0, r1};
      pl[1] = __builtin_bit_cast(unsigned, __builtin_convertvector(r, f16x2));
    }
  }
}

// one 32x32x16 product group: c += w * x on PM terms (small terms first)
template <int PM>
__device__ __forceinline__ void mma32(f32x16& c, const typename Prec<PM>::frag (&w)[Prec<PM>::NP],
                                      const typename Prec<PM>::frag (&x)[Prec<PM>::NP]) {
  if constexpr (PM == 3) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[1], x[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[2], x[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0], x[2], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[1], x[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0], x[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0], x[0], c, 0, 0, 0);
  } else if constexpr (PM == 2) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(w[1], x[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(w[0], x[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(w[0], x[0], c, 0, 0, 0);
  } else {
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(w[0], x[0], c, 0, 0, 0);
  }
}

// Power-of-two scaling of the fp16 modes: e such that amax * 2^e lies in [2^12, 2^13)
// (fp16 overflows at 2^16), clamped so that 2^-(ex + ew) stays a normal float.
__host__ __device__ __forceinline__ int dsm_amax_exponent(float amax) {
  const int ex = (int)((__builtin_bit_cast(unsigned, amax) >> 23) & 0xffu) - 127;
  const int e = 12 - ex;
  return e < -60 ? -60 : (e > 60 ? 60 : e);
}
__host__ __device__ __forceinline__ float dsm_pow2f(int e) {
  return __builtin_bit_cast(float, (unsigned)(e + 127) << 23);
}
// 2^e in a scalar register: the split's inline asm takes its factor as an "s" operand
__device__ __forceinline__ float dsm_pow2f_uniform(int e) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, dsm_pow2f(e))));
}

// scaling of a launch (PM < 3) from the two tensors' maxima: sx = 2^ex (wave-uniform) multiplies the staged
// activations, `out` = 2^-(ex + ew) is folded into the epilogue's scale
struct SplitScale { float sx, out; };
template <int PM>
__device__ __forceinline__ SplitScale split_scale(const float* x_amax, const float* w_amax) {
  if constexpr (PM == 3) return SplitScale{1.f, 1.f};
  else {
    const int ex = dsm_amax_exponent(*x_amax), ew = dsm_amax_exponent(*w_amax);
    return SplitScale{dsm_pow2f_uniform(ex), dsm_pow2f(-(ex + ew))};
  }
}

// ---- the tensor maxima: every f16x2 consumer trusts these slots blindly
// running max |v| of a thread's output quads: the running maximum is folded in with the first pair (the
// epilogues' form; one quad per call)
__device__ __forceinline__ void track_amax(float& am, const f32x4 v) {
  am = fmaxf(fmaxf(am, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
}
// max |v| of one quad by itself, for a caller that folds several quads into its maximum at once (spp.hip).
// The same value as track_amax gives -- a maximum does not depend on association -- but the association
// decides how many temporaries live: each caller keeps the one it was tuned with.
__device__ __forceinline__ float quad_amax(const f32x4 v) {
  return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
}

// max |y| of a launch, per workgroup of NWAVES (4 | 8) waves: one wave reduction, one LDS exchange between
// the waves and ONE atomic per workgroup (non-negative floats order like their bit patterns) -- and none at
// all when the slot already holds as much (hundreds of same-address atomics per launch serialise in L2).
// `lds`: NWAVES floats.  LDS_IN_USE: the floats alias LDS that other waves may still be reading (the
// kernels' tile images), so a barrier precedes the write; false for a dedicated __shared__ array.
template <int NWAVES, bool LDS_IN_USE = true>
__device__ __forceinline__ void publish_amax(float* slot, float am, float* lds) {
  static_assert(NWAVES == 4 || NWAVES == 8, "workgroups of four or eight waves");
  if (!slot) return;                                   // uniform
#pragma unroll
  for (int o = 32; o; o >>= 1) am = fmaxf(am, __shfl_xor(am, o));
  if constexpr (LDS_IN_USE) __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = am;
  __syncthreads();
  if (threadIdx.x == 0) {
    am = fmaxf(fmaxf(lds[0], lds[1]), fmaxf(lds[2], lds[3]));
    if constexpr (NWAVES == 8) am = fmaxf(am, fmaxf(fmaxf(lds[4], lds[5]), fmaxf(lds[6], lds[7])));
    if (am > __builtin_nontemporal_load(slot))
      atomicMax(reinterpret_cast<unsigned*>(slot), __builtin_bit_cast(unsigned, am));
  }
}

// The per-wave form of the element-wise passes (bn3d.hip): a wave reduction, then one atomic per wave -- and
// none once the slot holds as much (the blocks of an element-wise pass are many; most of them find the
// maximum already there).  No LDS and no barrier, so a kernel may publish several slots back to back.
// (The apply kernels walk their elements with a bounded grid, so a launch issues at most a few
// thousand of these: same-address atomics serialise in L2 at ~5 ns each.)
__device__ __forceinline__ void publish_amax_per_wave(float* slot, float am) {
  if (!slot) return;
#pragma unroll
  for (int o = 32; o; o >>= 1) am = fmaxf(am, __shfl_xor(am, o));
  if ((threadIdx.x & 63) == 0 && am > *reinterpret_cast<volatile float*>(slot))
    atomicMax(reinterpret_cast<unsigned*>(slot), __builtin_bit_cast(unsigned, am));
}

}  // namespace
