/*
 * dsmnet_hip.h -- C ABI of the MI355X (gfx950) stereo cost-volume path.
 *
 * The reference (sunshinnnn/DSMnet) is pure Python: it defines NO plugin,
 * operator or FFI interface for this path.  Each entry
 * point below therefore cites the reference *Python code it replaces*; the
 * binding a maintainer adds on the reference side is a ctypes stub
 * (INTEGRATION.md, and dsmnet_amd/_lib.py is that stub in full).
 *
 * Conventions
 *  - plain C: device pointers + sizes; no torch types, no C++ in the signatures;
 *  - every buffer is caller-allocated device memory; the library never
 *    allocates, frees, or synchronises; all work is enqueued on `stream`
 *    (a hipStream_t passed as void*; NULL = the null stream);
 *  - return value: DSM_OK (0) or a negative DSM_ERR_* code; no exceptions
 *    cross the boundary; dsm_strerror() names a code;
 *  - dtype: tensors are fp32 (DSM_F32; the reference computes in fp32: torch.FloatTensor,
 *    models/psmnet/stackhourglass.py:124).  What the convolutions MULTIPLY in is a per-call choice,
 *    dsm_conv3d_args.precision (DSM_PREC_*): fp32-accurate (default), or operands rounded to fp16
 *    with fp32 accumulation -- the reduced-precision mode of BASELINE config #5;
 *  - 4-D feature maps are NCHW contiguous, as torch hands them over;
 *  - 5-D volumes are either DSM_NCDHW (torch contiguous) or DSM_NDHWC
 *    (torch.channels_last_3d), selected per call.
 */
#ifndef DSMNET_HIP_H
#define DSMNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSM_ABI_VERSION 7

#define DSM_OK               0
#define DSM_ERR_ARG         -1   /* null pointer, non-positive size, bad enum      */
#define DSM_ERR_UNSUPPORTED -2   /* valid request this build has no kernel for     */
#define DSM_ERR_LAUNCH      -3   /* HIP reported a launch failure                   */
#define DSM_ERR_ALIGN       -4   /* a pointer is not aligned as the kernel needs    */

enum dsm_dtype  { DSM_F32 = 0 };
enum dsm_layout { DSM_NCDHW = 0, DSM_NDHWC = 1 };

typedef void* dsm_stream_t;      /* hipStream_t */

int         dsm_abi_version(void);
const char* dsm_strerror(int code);

/* ---------------------------------------------------------------------------
 * (a1) 1-D correlation.  Replaces Corr1d.forward, models/util_conv.py:71-86
 * (python loop over D slice-multiplies) and, for the gradient, autograd through it.
 *   out[b,i,y,x] = sum_c fL[b,c,y,x] * fR[b,c,y,x - i*stride]   (x >= i*stride, i < W)
 *   ksize > 1: every plane box-filtered, zero padding counted in the divisor
 *   (nn.AvgPool2d(k, 1, k//2), util_conv.py:82-85).
 * fL, fR: (B,C,H,W); out: (B,D,H,W); tmp: (B,D,H,W) scratch, needed iff ksize > 1.
 * ------------------------------------------------------------------------- */
int dsm_corr1d_fwd(const void* fL, const void* fR, void* out, void* tmp,
                   int B, int C, int H, int W, int D, int stride, int ksize,
                   int dtype, dsm_stream_t stream);

/* (ABI v7, additive) Host-only plan queries of the ops that choose between several kernels.  Each
 * takes the arguments of the entry point it describes (the stream replaced by buf, len), runs the
 * SAME selection code as the launch, returns the SAME error codes the launch would return, and
 * writes the NUL-terminated name of the chosen branch into buf[len].  Pointers are inspected for
 * NULL and 16-byte alignment only, never dereferenced: no launch, no device access, no GPU needed.
 *
 * dsm_corr1d_plan:  "tile<S,NDH>"  the all-channels-in-LDS tile kernel (S = stride 1 | 2; NDH = 1 for
 *                                  D <= 48, 2 for D <= 96); needs 16-byte accesses, C % 16 == 0 and
 *                                  a window of at most 150 KB - 4 KB of LDS;
 *                   "fwd<S>vec" / "fwd<S>scalar"  the chunked kernel (stride 1 | 2, D <= 128), with
 *                                  16-byte or scalar global accesses (W % 4 != 0 or a pointer that
 *                                  is not 16-byte aligned: scalar);
 *                   "generic"      one thread per output (any other stride, D > 128);
 *   followed by "+box3" (ksize 3, 16-byte accesses) or "+box" (any other ksize > 1). */
int dsm_corr1d_plan(const void* fL, const void* fR, const void* out, const void* tmp,
                    int B, int C, int H, int W, int D, int stride, int ksize,
                    int dtype, char* buf, int len);

/* grad_out: (B,D,H,W); dfL, dfR: (B,C,H,W), fully overwritten.
 * tmp: (B,D,H,W) scratch, needed iff ksize > 1. */
int dsm_corr1d_bwd(const void* grad_out, const void* fL, const void* fR,
                   void* dfL, void* dfR, void* tmp,
                   int B, int C, int H, int W, int D, int stride, int ksize,
                   int dtype, dsm_stream_t stream);

/* (ABI v7, additive) Corr1d with a similarity argument (the `simfun` of util_conv.py:57-66) and the tiled
 * data gradient.  dsm_corr1d_fwd / _bwd / _plan above are unchanged; DSM_SIM_DOT here runs their kernels.
 *
 * DSM_SIM_COSINE is nn.CosineSimilarity(dim=1, eps) per plane, each norm clamped on its own
 * (F.cosine_similarity of torch >= 1.12; PyTorch 0.3 clamped the product of the two norms):
 *   a(b,y,x) = 1 / max(||fL[b,:,y,x]||, eps),   r(b,y,x) = 1 / max(||fR[b,:,y,x]||, eps),   x' = x - i*stride
 *   raw[b,i,y,x] = a(x) r(x') sum_c fL[b,c,y,x] fR[b,c,y,x']      (x' >= 0, else 0)
 *   out = raw (ksize 1) or the box filter of raw (ksize > 1), as for the dot product.
 * Gradients are those of this formula with a clamped norm held constant: with g = box(grad_out) and
 * g'_i(x) = g_i(x) a(x) r(x'),
 *   dfL[c,x ] = sum_i g'_i(x)          fR[c,x - i s]   - [||fL(x)|| >= eps]  a(x)^2  fL[c,x]  sum_i g_i(x) raw_i(x)
 *   dfR[c,x'] = sum_i g'_i(x' + i s)   fL[c,x' + i s]  - [||fR(x')|| >= eps] r(x')^2 fR[c,x'] sum_i g_i(x'+i s) raw_i(x'+i s)
 * i.e. the dot-product backward applied to g', one pass in front and one term in the epilogue.
 *
 * Forward.  raw: (B,D,H,W), needed iff ksize > 1 (the unfiltered map; the cosine backward reads it).
 * inv: (2,B,H,W) floats, needed iff DSM_SIM_COSINE, written here: a, then r.  eps > 0 (ignored for the dot
 * product).  Cosine: 2 launches (ksize 1) or 3; no pass over the (B,D,H,W) map is added.
 * Extents the cosine passes cannot index (B*H*W or W + D*stride above 2^31 - 1) are DSM_ERR_UNSUPPORTED.
 * Plan names: those of dsm_corr1d_plan, cosine with the prefix "cos:" ("cos:tile<1,1>+box3"); inv counts
 * among the pointers that 16-byte accesses need aligned. */
enum dsm_corr_sim { DSM_SIM_DOT = 0, DSM_SIM_COSINE = 1 };

int dsm_corr1d_sim_fwd(const void* fL, const void* fR, void* out, void* raw, void* inv,
                       int B, int C, int H, int W, int D, int stride, int ksize,
                       int sim, float eps, int dtype, dsm_stream_t stream);
int dsm_corr1d_sim_fwd_plan(const void* fL, const void* fR, const void* out, const void* raw,
                            const void* inv, int B, int C, int H, int W, int D, int stride, int ksize,
                            int sim, float eps, int dtype, char* buf, int len);

/* Backward.  raw_or_out: the forward's raw map (ksize > 1) or its out (ksize 1), and inv: the forward's;
 * both needed iff DSM_SIM_COSINE.  dfL, dfR: (B,C,H,W), fully overwritten.  workspace: at least
 * dsm_corr1d_sim_workspace_bytes(...) bytes, needed iff that is not 0.
 * flags: DSM_CORR_BWD_NAIVE forces the one-thread-per-element kernel of dsm_corr1d_bwd (A/B runs).
 * Plan names: "bwd_tile<S>" (S = stride 1 | 2; needs W % 4 == 0, D <= 96, at most 150 KB of LDS and fL, fR,
 * dfL, dfR, the gradient it reads -- grad_out, or the workspace when ksize > 1 or cosine -- 16-byte aligned)
 * or "bwd_naive"; in front "prep+" (cosine: g' and the two sums) and before that "box3+" (ksize 3, W % 4 == 0,
 * grad_out and workspace 16-byte aligned) or "box+" (any other ksize > 1).  No atomics anywhere: results
 * are bit-reproducible. */
#define DSM_CORR_BWD_NAIVE 1

int dsm_corr1d_sim_bwd(const void* grad_out, const void* fL, const void* fR,
                       const void* raw_or_out, const void* inv, void* dfL, void* dfR, void* workspace,
                       int B, int C, int H, int W, int D, int stride, int ksize,
                       int sim, float eps, int flags, int dtype, dsm_stream_t stream);
int dsm_corr1d_sim_bwd_plan(const void* grad_out, const void* fL, const void* fR,
                            const void* raw_or_out, const void* inv, const void* dfL, const void* dfR,
                            const void* workspace, int B, int C, int H, int W, int D, int stride, int ksize,
                            int sim, float eps, int flags, int dtype, char* buf, int len);
size_t dsm_corr1d_sim_workspace_bytes(int B, int C, int H, int W, int D, int ksize, int sim);

/* ---------------------------------------------------------------------------
 * (a2,a3) concatenation cost volume.  Replaces the inline loops of
 * models/gcnet.py:130-135 (mask_left = 0) and
 * models/psmnet/stackhourglass.py:124-133 (mask_left = 1):
 *   vol[b,   c, d,y,x] = fL[b,c,y,x]        (x >= d, or every x when !mask_left)
 *   vol[b, C+c, d,y,x] = fR[b,c,y,x - d]    (x >= d)          zero elsewhere
 * fL, fR: (B,C,H,W); vol: (B,2C,D,H,W) in `layout`; written in one pass, no memset.
 * mask_left bit 1 (ABI v4, NDHWC forward only): the right-referenced volume of gcnet_LR
 * (models/gcnet.py:155-164) -- pass (fR, fL) as (fL, fR): the second map is read at x + d,
 *   vol[b, C+c, d,y,x] = second[b,c,y,x + d]   (x + d < W), zero elsewhere.
 * ------------------------------------------------------------------------- */
int dsm_concat_volume_fwd(const void* fL, const void* fR, void* vol,
                          int B, int C, int H, int W, int D,
                          int mask_left, int layout, int dtype, dsm_stream_t stream);

/* gvol: (B,2C,D,H,W) in `layout`; dfL, dfR: (B,C,H,W), fully overwritten. */
int dsm_concat_volume_bwd(const void* gvol, void* dfL, void* dfR,
                          int B, int C, int H, int W, int D,
                          int mask_left, int layout, int dtype, dsm_stream_t stream);

/* (ABI v7, additive) Plan queries (see dsm_corr1d_plan).  Forward: "ndhwc", "ndhwc lds>64K" (the
 * staged rows need more than 64 KB of LDS: the kernel's limit is raised first; more than 160 KB is
 * DSM_ERR_UNSUPPORTED), "ncdhw vec" (W % 4 == 0 and vol 16-byte aligned), "ncdhw scalar".
 * Backward: "ndhwc_bwd", "ncdhw_bwd". */
int dsm_concat_volume_fwd_plan(const void* fL, const void* fR, const void* vol,
                               int B, int C, int H, int W, int D,
                               int mask_left, int layout, int dtype, char* buf, int len);
int dsm_concat_volume_bwd_plan(const void* gvol, const void* dfL, const void* dfR,
                               int B, int C, int H, int W, int D,
                               int mask_left, int layout, int dtype, char* buf, int len);

/* ---------------------------------------------------------------------------
 * (a6,a7) soft-argmin disparity regression, fused.  Replaces
 *   PSMNet: F.upsample(trilinear) -> F.softmax -> disparityregression
 *           (stackhourglass.py:152-166, submodule.py:56-63):  negate = 0,
 *           cost (B,Dc,Hc,Wc) upsampled to (D,H,W) on the fly;
 *   GCNet:  Softmax2d(-x) -> matmul(arange) (models/gcnet.py:104-111): negate = 1,
 *           (Dc,Hc,Wc) == (D,H,W), no interpolation.
 *   disp[b,y,x] = sum_d d * softmax_d(+-cost_up[b,d,y,x])
 * cost: (B,Dc,Hc,Wc); disp: (B,H,W); stats: (B,2,H,W) or NULL -- per-pixel
 * softmax max and normaliser, saved for the backward pass.
 * align_corners follows torch.nn.functional.interpolate (0 = what F.upsample
 * resolves to on torch >= 0.4; see DESIGN.md "version drift").
 * ------------------------------------------------------------------------- */
int dsm_soft_argmin_fwd(const void* cost, void* disp, void* stats,
                        int B, int Dc, int Hc, int Wc, int D, int H, int W,
                        int negate, int align_corners, int dtype, dsm_stream_t stream);

/* gdisp: (B,H,W); dcost: (B,Dc,Hc,Wc), fully overwritten (zeroed on `stream`
 * first when the upsampling adjoint accumulates into it). */
int dsm_soft_argmin_bwd(const void* cost, const void* disp, const void* stats,
                        const void* gdisp, void* dcost,
                        int B, int Dc, int Hc, int Wc, int D, int H, int W,
                        int negate, int align_corners, int dtype, dsm_stream_t stream);

/* (ABI v7, additive) Plan queries (see dsm_corr1d_plan).  Forward: "up4<4>" (the x4 head: D == 4 Dc,
 * align_corners = 0, Dc >= 4), "fwd<true,DS>" (interpolating) or "fwd<false,DS>" (GCNet form) with
 * DS = 4 | 2 | 1 lane segments per pixel (D >= 8 | D >= 4 | D < 4).  Backward: "bwd_direct" (no
 * interpolation), "bwd_tile nseg=N" (the LDS-tiled adjoint; N = 1 | 2 | 4 disparity segments for
 * D < 16 | D < 96 | D >= 96), "bwd_fallback" (per-pixel global atomics: the coarse box of a 32 x 8
 * tile needs more than 48 KB of LDS -- down-sampling -- or B * N > 65535). */
int dsm_soft_argmin_fwd_plan(const void* cost, const void* disp, const void* stats,
                             int B, int Dc, int Hc, int Wc, int D, int H, int W,
                             int negate, int align_corners, int dtype, char* buf, int len);
int dsm_soft_argmin_bwd_plan(const void* cost, const void* disp, const void* stats,
                             const void* gdisp, const void* dcost,
                             int B, int Dc, int Hc, int Wc, int D, int H, int W,
                             int negate, int align_corners, int dtype, char* buf, int len);

/* (ABI v7, additive) Confidence heads: the distribution dsm_soft_argmin_fwd regresses from, kept for
 * four more per-pixel maps, in one launch.  Inputs as dsm_soft_argmin_fwd; with v_d the sign times the
 * interpolated cost, p = softmax(v), d* the smallest d with v_d = max v and the window
 * Wn = [max(0, d* - radius), min(D - 1, d* + radius)], all maps (B,H,W) fp32:
 *   disp    = sum_d d p_d            (what dsm_soft_argmin_fwd writes)
 *   pmax    = p_{d*}                   pwin = sum_{Wn} p_d
 *   peak    = sum_{Wn} d p_d / pwin    (the regression restricted to the window around the arg-max)
 *   entropy = -sum_d p_d ln p_d        (nats, in [0, ln D])
 * Any of peak, pmax, pwin, entropy may be NULL and is then skipped; radius >= 0 (DSM_ERR_ARG otherwise),
 * radius >= D - 1 gives pwin = 1 and peak = disp.  Wherever both interpolation indices along d coincide
 * (the clamped top end) the fine value is the plane's own value, bit for bit, so the equal end bins of the
 * D = 4 Dc head resolve to the lower one by rule, not by rounding.  Forward only; no host read, no
 * allocation, capturable.  Plan: "conf_up4<4>", "conf<true,DS>", "conf<false,DS>", chosen as the
 * soft-argmin forward's. */
int dsm_disp_confidence_fwd(const void* cost, void* disp, void* peak, void* pmax, void* pwin, void* entropy,
                            int B, int Dc, int Hc, int Wc, int D, int H, int W,
                            int negate, int align_corners, int radius, int dtype, dsm_stream_t stream);
int dsm_disp_confidence_fwd_plan(const void* cost, const void* disp, const void* peak, const void* pmax,
                                 const void* pwin, const void* entropy,
                                 int B, int Dc, int Hc, int Wc, int D, int H, int W,
                                 int negate, int align_corners, int radius, int dtype, char* buf, int len);

/* ---------------------------------------------------------------------------
 * (a4,a5) 3-D convolution block, k = 3, fused epilogue.  Replaces
 *   convbn_3d (+ReLU, +skip)            models/psmnet/submodule.py:16-19,
 *                                       stackhourglass.py:22-62,73-98,135-149
 *   conv3d_bn / deconv3d_bn             models/util_conv.py:150-179,
 *   myadd_3d / myAdd3d (crop + add)     stackhourglass.py:10-20, util_fun.py:41-50
 *   relu = 1:  y = relu( conv(x, w) * scale[co] + shift[co]  (+ residual, cropped) )   PSMNet order
 *   relu = 2:  y = relu( conv(x, w) * scale[co] + shift[co] )  (+ residual, cropped)   GCNet order
 *              (models/gcnet.py:78-96: the ReLU sits inside deconv3d_bn, myAdd3d follows)
 *   relu = 0:  no activation
 * `scale`/`shift` carry the folded eval-mode BatchNorm and the conv bias.
 * transposed = 0: Conv3d(k=3, padding=1, stride in {1,2})
 * transposed = 1: ConvTranspose3d(k=3, stride=2, padding=1, output_padding=1)
 * Activations are DSM_NDHWC, fp32.  (Do,Ho,Wo) may be smaller than the natural
 * output size: only that corner is computed -- this is the crop of myadd_3d.
 * The contraction runs in the mode `precision` names (DSM_PREC_* below): split 16-bit operands on the bf16 /
 * fp16 MFMAs with fp32 accumulation, or -- DSM_CONV_FP32_MFMA, and every layer no split kernel covers -- fp32
 * operands on v_mfma_f32_32x32x2_f32.  Products are exact only in that last form; sums are rounded to fp32
 * after every MFMA in all of them.
 * ------------------------------------------------------------------------- */
typedef struct dsm_conv3d_args {
  const void*  x;         /* (B,Di,Hi,Wi,Cin)                                   */
  const void*  w_packed;  /* from dsm_conv3d_pack_weights                        */
  const float* scale;     /* [Cout] or NULL (= 1)                                */
  const float* shift;     /* [Cout] or NULL (= 0)                                */
  const void*  residual;  /* (B,Dr,Hr,Wr,Cout) or NULL                           */
  void*        y;         /* (B,Do,Ho,Wo,Cout)                                   */
  int B, Cin, Cout;
  int Di, Hi, Wi;
  int Do, Ho, Wo;
  int Dr, Hr, Wr;
  int stride;
  int transposed;
  int relu;               /* 0 none, 1 after the skip add, 2 before it */
  /* kernel geometry; 0 = default.  kd = 1 selects the 2-D form (Di = Do = 1, NHWC maps as
   * (B,1,H,W,C) volumes) used for the 2-D feature towers:
   * k in {1,3}, dil in {1,2}, padding = dil*(k-1)/2 ("same"), as in convbn()
   * (models/psmnet/submodule.py:10-13) for k = 3 and the towers' 1x1 convolutions. */
  int kd;                 /* depth taps: 3 (default) or 1            */
  int k;                  /* taps in y and x: 3 (default) or 1; 5: see "5x5 stride-2 layers" below */
  int dil;                /* dilation in y and x: 1 (default) or 2   */
  /* ABI v4: tuning / A-B switches of THIS call (0 = the plan's own choice).  The library reads no
   * environment variable and holds no global switch: a plan is a pure function of the arguments. */
  int          flags;
  /* ABI v6: what the 3x3(x3) MFMA kernels multiply in (DSM_PREC_*, below).  The fp16 modes scale
   * every tensor by a power of two taken from its absolute maximum: `x_amax` points at a device
   * float holding max |x| (or an upper bound of it) -- written by the launch that produced x
   * through ITS y_amax, or by dsm_absmax; required when precision != DSM_PREC_F32 and the layer runs
   * on a split kernel (dsm_conv3d_plan names it "..._f16x2_..." / "..._f16_..."), ignored otherwise.
   * The names are a contract: the Python host layer decides from them whether to hand x_amax over. */
  int          precision;
  const float* x_amax;
  /* ABI v6: optional.  max |y| of this launch is folded into *y_amax with an atomic maximum on the
   * float bits: the caller zeroes it (on the stream) before the launch.  Any precision, every MFMA
   * kernel (Cout >= 32). */
  float*       y_amax;
  /* ABI v6: vol_virtual = 1 -- the input is a concatenation cost volume that is NEVER MATERIALISED
   * (models/psmnet/stackhourglass.py:124-133 with vol_mask_left = 1, models/gcnet.py:130-135 with 0,
   * fused into the first 3-D convolution).  `x` is then the NHWC feature tensor (2B, Hi, Wi, Cin/2)
   * [the B left maps, then the B right maps]; input plane d of the (B, Cin, Di, Hi, Wi) volume is
   * staged as [left | right shifted by d voxels] with x < d zeroed (right half always, left half
   * iff vol_mask_left); Di = the number of disparity planes.  Conv3d(k3, s1) to 32 channels only
   * (the z-sliding kernel, "conv3d_zs_..."): DSM_ERR_UNSUPPORTED otherwise.  x_amax: of the features. */
  int          vol_virtual;
  int          vol_mask_left;
  /* (ABI v7, additive) Scratch of the kernels that split the contraction over workgroups -- the wide 2-D
   * layers, "conv2d_wide_..." with a split count above 1: dsm_conv3d_workspace_bytes(args) bytes of device
   * memory, 16-byte aligned, contents undefined before and after the call; NULL / 0 where that query
   * returns 0.  Too small or missing: DSM_ERR_ARG, nothing launched. */
  void*        workspace;
  size_t       workspace_bytes;
} dsm_conv3d_args;
/* fp32 operands, fp32-accurate products and sums: three-term bf16 split (six bf16 MFMAs per
 * product) or, with DSM_CONV_FP32_MFMA, the fp32-input MFMA */
#define DSM_PREC_F32    0
/* operands rounded to fp16 (after the power-of-two scaling), one MFMA per product, fp32 accumulate:
 * relative error ~3e-4 of the result's scale.  BASELINE config #5 ("fp16 training step"). */
#define DSM_PREC_F16    1
/* fp32 accuracy on the fp16 pipe: x * 2^e = hi + lo in fp16 (22 significand bits), three MFMAs per
 * product (wl xh + wh xl + wh xh), fp32 accumulate; measured error vs float64 at or below the
 * bf16x3 and fp32-input kernels' (scripts/precision_check.py).
 * Supported range: a tensor's maximum (x_amax, max |w|) in [2^-48, 2^76) -- below it the exponent's clamp
 * (+-60) leaves the scaled values short of 2^12 and bits are lost, from 2^76 the scaled maximum overflows fp16.
 * Accuracy is relative to that maximum, not to each element: an operand element carries an absolute error of
 * up to 2^-37 of its tensor's maximum (half an fp16 subnormal step against a maximum scaled to 2^12), so it
 * keeps 22 bits only down to about 2^-14 of the maximum (tests/split_bound.py states the per-output bound,
 * tests/test_split_contract_gpu.py holds every kernel to it). */
#define DSM_PREC_F16X2  2
#define DSM_CONV_FP32_MFMA      0x1      /* keep the layer on the exact fp32-input MFMA (no bf16x3)   */
#define DSM_CONV_COUT1_CHUNKED  0x2      /* Cout = 1: the chunked kernel instead of the z-sliding one */
#define DSM_CONV_NO_NSPLIT      0x4      /* 2-D bf16x3 layers: one workgroup per tile (no N-split)    */
#define DSM_CONV_NO_ONCE        0x8      /* A/B: the chunk-pipelined single-kind kernels instead of the single-tile (2-D 64 -> 64) and two-kind (stride-2 3-D) forms */
#define DSM_CONV_KSPLIT_SHIFT   8        /* bits 8..13: wide 2-D and 5x5 stride-2 layers: force the number of K-ranges (1..63, clamped to [ceil(Cin / 128), Cin / 16]) */
#define DSM_CONV_TM_SHIFT       4        /* bits 4..7: force the tile height 4*TM rows (TM = 1, 2, 4) */
#define DSM_CONV_BLOCKS_SHIFT   16       /* bits 16..31: force the persistent grid size               */

/* bytes of the packed (MFMA-fragment-ordered) weight buffer */
size_t dsm_conv3d_packed_weight_bytes(int Cin, int Cout, int transposed);

/* w_torch: torch layout, (Cout,Cin,3,3,3) or, transposed, (Cin,Cout,3,3,3). */
int dsm_conv3d_pack_weights(const void* w_torch, void* w_packed,
                            int Cin, int Cout, int transposed, dsm_stream_t stream);

/* General packer: kd x k x k taps, torch layout (Cout, Cin_src, [kd,] k, k); input channels
 * Cin_src..Cin-1 are packed as zeros (PSMNet's first convolution: 3 staged as 16).
 * Bytes needed: dsm_conv_packed_weight_bytes (the fp32 fragments, Cin*Cout*kd*k*k*4, followed for
 * 3x3(x3) kernels by the pre-split bf16 planes the bf16x3 kernels read and by the two fp16 planes
 * of the power-of-two-scaled weights behind a 16-byte header holding their absolute maximum).
 * kd = 1, k = 5 (Cout 128 | 256, Cin % 16 == 0; every other 5x5 shape: 0 bytes, DSM_ERR_UNSUPPORTED): the
 * header and the two fp16 planes ALONE, 16 + Cin*Cout*25*4 bytes. */
size_t dsm_conv_packed_weight_bytes(int Cin, int Cout, int kd, int k);
int dsm_conv_pack_weights(const void* w_torch, void* w_packed, int Cin_src, int Cin, int Cout,
                          int kd, int k, dsm_stream_t stream);

/* (ABI v6) max |x| over n floats, folded into *amax (atomic maximum on the float bits; the caller
 * zeroes it first): the `x_amax` of a tensor no launch of this library produced. */
int dsm_absmax(const void* x, size_t n, float* amax, dsm_stream_t stream);

/* Two convolutions per launch: the stride-1 BasicBlock of PSMNet's towers (models/psmnet/submodule.py:24-46;
 * C = 64 or 32) and of GCNet's (models/util_conv.py:181-210; C = 32, relu = 1):
 * y = [ReLU](BN2(conv2(ReLU(BN1(conv1(x))))) + x),  both Conv2d(C, C, 3, stride 1, pad 1), folded BatchNorm as
 * scale / shift per channel (NULL: 1 / 0); relu = 1: ReLU after the skip add.  x, y: fp32 NHWC (B, H, W, C);
 * w1_packed, w2_packed: dsm_conv_pack_weights buffers of the two layers (Cin = Cout = C, kd = 1, k = 3).  precision: DSM_PREC_F16X2 or DSM_PREC_F16 (the fp16 modes only); x_amax as in
 * dsm_conv3d_args (required), y_amax optional.  The intermediate map never leaves the chip; it is scaled
 * for its fp16 split by each tile's own maximum.  Eval mode only (no backward). */
typedef struct {
  const void* x; void* y;
  const void* w1_packed; const void* w2_packed;
  const float* scale1; const float* shift1; const float* scale2; const float* shift2;
  const float* x_amax; float* y_amax;
  int B, H, W, C;
  int precision;
  int relu;
  int no_skip;       /* 1: no `+ x` (two convolution + BN + ReLU layers in a row: PSMNet's firstconv) */
} dsm_basicblock2d_args;
int dsm_basicblock2d_fwd(const dsm_basicblock2d_args* a, dsm_stream_t stream);

int dsm_conv3d_fwd(const dsm_conv3d_args* args, dsm_stream_t stream);

/* (ABI v7, additive) Wide 2-D layers -- Conv2d(k3, pad 1, stride 1 | 2) to Cout = 256 | 512 | 1024 from
 * Cin % 16 == 0 (kd = 1, k = 3, dil = 1, no residual, natural output size), the encoder of DispNetC / iResNet
 * (models/dispnetcorr.py:37-45 conv3b .. conv6b, models/iresnet.py conv3_1 .. conv6_1: conv2d_bn with
 * bn = False, models/util_conv.py) -- run on "conv2d_wide_<f16x2|f16>_mfma_kernel<S,N,KS=K,units>": precision
 * DSM_PREC_F16X2 or DSM_PREC_F16 only (DSM_PREC_F32, or DSM_CONV_FP32_MFMA: DSM_ERR_UNSUPPORTED -- the caller
 * keeps its own layer).  The contraction (9 Cin) is cut into K ranges of 16-channel chunks, one workgroup
 * each per (pixel block, N = 64 | 32 output channels); K > 1: the partial sums meet in `workspace`
 * ([K][B*Ho*Wo][Cout] floats) and a second launch adds them in index order (no float atomics: the
 * result is bit-identical from run to run; different K differ in the low bits).  This query: the bytes
 * `workspace` must hold for `args` (flags included); 0 when the layer needs none or is not such a layer.
 *
 * (ABI v7, additive) 5x5 stride-2 layers -- Conv2d(k5, pad 2, stride 2) to Cout = 128 | 256 from Cin % 16 == 0
 * (kd = 1, k = 5, stride = 2, dil = 1, no residual, the natural output size Ho = (Hi - 1) / 2 + 1), conv2 and
 * conv3a of DispNet (models/dispnet.py:26-27) and the conv2 of DispNetC / iResNet -- run on
 * "conv2d_k5_<f16x2|f16>_mfma_kernel<S=2,N,KS=K,units>", the same kernel with a 5x5 window: the same
 * precisions (DSM_PREC_F32, or DSM_CONV_FP32_MFMA: DSM_ERR_UNSUPPORTED), the same K ranges, `workspace`
 * rule, deterministic second launch and `flags` bits, x_amax required (DSM_ERR_ARG without), y_amax folded
 * in.  Stride 1, dilation 2, other Cout, a residual, a cropped output, an output wider than 592 columns
 * (eight column blocks of one staged box) and maps past the 32-bit offsets are DSM_ERR_UNSUPPORTED.
 * w_packed: dsm_conv_pack_weights(..., kd = 1, k = 5), dsm_conv_packed_weight_bytes(Cin, Cout, 1, 5) =
 * 16 + Cin * Cout * 25 * 4 bytes -- a 16-byte header {max |w|, 0, 0, 0} and the two fp16 planes
 * [Cin/16][tap 25][Cout/32][plane][lane][16 B]; these layers have no fp32 and no bf16 section. */
size_t dsm_conv3d_workspace_bytes(const dsm_conv3d_args* args);

/* Name of the kernel variant dsm_conv3d_fwd would launch for `args` (tile shape and
 * channel chunk are chosen per layer) -- written NUL-terminated into buf[len];
 * used by bench.py to attribute per-launch timings.  No launch, no device access.
 * Returns the SAME error codes the launch would return for `args` (as the corr1d, soft-argmin and volume
 * queries do): the plan, dsm_conv3d_workspace_bytes and dsm_conv3d_fwd share one selection, and a variant
 * that is not compiled (say Conv2d(k3, dilation 2) to 32 or 64 channels on the split kernels) is
 * DSM_ERR_UNSUPPORTED here, with buf = "", not a name.  The launch's alone: a missing or short `workspace`
 * of the wide layers (DSM_ERR_ARG), DSM_ERR_LAUNCH from the runtime, and the launchers' own tile-count bounds,
 * which no extent under the plan's 4 GiB bound reaches. */
int dsm_conv3d_plan(const dsm_conv3d_args* args, char* buf, int len);

/* (ABI v7, additive) The transposed mode of the wide 2-D kernel: backward-data of the stride-2 wide layers.
 * dsm_conv3d_args with kd = 1, k = 3, dil = 1, transposed = 1, stride = 2, Cout = 256 | 512 | 1024,
 * Cin % 16 == 0, precision DSM_PREC_F16X2 | DSM_PREC_F16 (else DSM_ERR_UNSUPPORTED, as for the wide layers;
 * every other transposed 2-D request stays DSM_ERR_UNSUPPORTED).  x: (B, Hi, Wi, Cin) NHWC; y: (B, Ho, Wo, Cout)
 * with 2 Hi - 1 <= Ho <= 2 Hi and 2 Wi - 1 <= Wo <= 2 Wi -- the extent of the tensor whose gradient this is.
 * With X' the zero-interleaved map of Ho x Wo (X'[2i][2j] = x[i][j], zero elsewhere):
 *   y = conv2d(X', w_packed, stride 1, pad 1), then scale / shift / ReLU and y_amax as usual,
 * which equals conv_transpose2d(x, W, stride 2, padding 1, output_padding 1)[:, :, :Ho, :Wo] when w_packed
 * holds the 180-degree-flipped, in/out-transposed W (dsm_conv_pack_weights, Cin = this Cin, Cout = this Cout).
 * Runs on "deconv2d_wide_<f16x2|f16>_mfma_kernel<N,KS=K,units>": the stride-1 work decomposition over
 * Ho x Wo, the same K ranges, `workspace` ([K][B*Ho*Wo][Cout] floats, dsm_conv3d_workspace_bytes) and the
 * same deterministic second launch; x_amax is required. */

/* (ABI v7, additive) Backward of bias + ReLU behind a wide layer, NHWC tensors viewed as [M][C], C % 4 == 0:
 *   g[m][c] = y[m][c] > 0 ? gy[m][c] : 0   (g is a tensor of its own; gy is never written)
 *   db[c]   = sum_m g[m][c]                (db may be NULL)
 *   *g_amax = max(*g_amax, max |g|)        (folded like y_amax of the convolutions; may be NULL)
 * One pass of 12 bytes per element plus a small second launch for db.  db is summed in a fixed order
 * (per-workgroup partial sums in `ws`, plain stores, then added in index order; no float atomics): two
 * runs give the same bits.  ws: min(512, ceil(M / 8)) * C floats -- 512 * C always suffices -- 16-byte
 * aligned; not read when db is NULL.  All tensors 16-byte aligned. */
int dsm_bias_relu_bwd(const void* gy, const void* y, void* g, void* db, void* ws, float* g_amax,
                      long M, int C, dsm_stream_t stream);

/* ---------------------------------------------------------------------------
 * Backward of the 3-D convolution blocks (training through the trunk; in the reference this
 * is autograd through nn.Conv3d / nn.ConvTranspose3d).  bwd-data is a convolution again and
 * runs on dsm_conv3d_fwd with re-packed weights (see dsmnet_amd/costvolume.py); these are the
 * bwd-weight entry points.
 *   dW[g][c][tap] = sum_v X[v*stride + tap - 1][c] * G[v][g]
 * x: (B,Dx,Hx,Wx,Cx) NDHWC, the strided-over side; g: (B,Dg,Hg,Wg,Cg) NDHWC.
 *   Conv3d(stride s):      X = layer input, G = dY        -> dw is (Cout, Cin, 3,3,3)
 *   ConvTranspose3d(s=2):  X = dY, G = layer input, stride 2 -> dw is (Cin, Cout, 3,3,3)
 * ws: scratch of (Cx/32)*(Cg/32)*27*1024 floats; dw: Cg*Cx*27 floats, overwritten.
 * Channels must be multiples of 32.  Sums are accumulated with fp32 atomics (order varies).
 * flags (ABI v5): DSM_CONV_FP32_MFMA keeps the exact fp32-input MFMA kernel; 0 = fp32 operands on
 * the 16-bit matrix pipe, staged once as [voxel][channel] 16-bit planes and read through gfx950's
 * transposed LDS read.  precision (ABI v6, DSM_PREC_*): bf16x3 (DSM_PREC_F32), or the fp16 forms
 * f16x2 / f16, which scale X and G by powers of two taken from the device scalars x_amax / g_amax
 * (max |X|, max |G|; required then -- dsm_absmax or a producer's y_amax).
 * flags bits 16..31 (DSM_CONV_BLOCKS_SHIFT), when not zero, force the number of persistent workgroups
 * per 32 x 32 channel pair (clamped to [1, work units]; tests walk long ranges with it); 0 keeps the
 * launcher's own choice, min(256 / pairs, units).
 * ------------------------------------------------------------------------- */
int dsm_conv3d_wgrad(const void* x, const void* g, void* ws, void* dw, int B, int Cx, int Cg,
                     int Dx, int Hx, int Wx, int Dg, int Hg, int Wg, int stride, int flags,
                     int precision, const float* x_amax, const float* g_amax, dsm_stream_t stream);

/* (ABI v5) The same for the 2-D towers' 3x3 layers -- autograd through convbn / BasicBlock
 * (models/psmnet/submodule.py:10-13,24-46) when the feature extraction trains.  padding = dilation;
 * (stride, dilation) in {(1,1), (1,2), (2,1)}.  x: (B,Hx,Wx,Cx) NHWC, g: (B,Hg,Wg,Cg) NHWC;
 * ws: (Cx/32)*(Cg/32)*9*32*32 floats (zeroed here); dw: (Cg, Cx, 3, 3) torch layout, overwritten.
 * flags: as for dsm_conv3d_wgrad, the forced grid size in bits 16..31 included. */
int dsm_conv2d_wgrad(const void* x, const void* g, void* ws, void* dw, int B, int Cx, int Cg,
                     int Hx, int Wx, int Hg, int Wg, int stride, int dilation, int flags,
                     int precision, const float* x_amax, const float* g_amax, dsm_stream_t stream);

/* Cout = 1, stride 1 (classifier heads): g (B,D,H,W); x (B,D,H,W,C); w_packed [27][C];
 * dx (B,D,H,W,C) or NULL; dw_tapmajor [27][C] or NULL (the caller transposes to (1,C,27)).
 * w_packed and dx must be 16-byte aligned when dx is asked for (DSM_ERR_ALIGN, nothing launched). */
int dsm_conv3d_cout1_bwd(const void* x, const void* g, const void* w_packed, void* dx,
                         void* dw_tapmajor, int B, int C, int D, int H, int W,
                         dsm_stream_t stream);

/* ConvTranspose3d(C -> 1, k3, s2, p1, op1) backward -- GCNet's head l37 (models/gcnet.py:63,98;
 * autograd through nn.ConvTranspose3d in the reference).  g (B,Do,Ho,Wo); x (B,Di,Hi,Wi,C)
 * NDHWC; w: torch layout (C,1,3,3,3); dx (B,Di,Hi,Wi,C) or NULL; dw (C,1,3,3,3) or NULL,
 * overwritten.  C % 4 == 0, C <= 256; dx 16-byte aligned (DSM_ERR_ALIGN, nothing launched). */
int dsm_deconv3d_cout1_bwd(const void* x, const void* g, const void* w, void* dx, void* dw,
                           int B, int C, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                           dsm_stream_t stream);

/* ---------------------------------------------------------------------------
 * Train-mode BatchNorm3d + cropped skip addition + ReLU on NDHWC fp32 volumes, forward and
 * backward (dsmnet_amd/csrc/bn3d.hip) -- what convbn_3d / conv3d_bn leave to nn.BatchNorm3d,
 * myadd_3d and F.relu in a training step of the reference (models/psmnet/submodule.py:16-19,
 * stackhourglass.py:10-20,43-62, models/util_conv.py:150-179, util_fun.py:41-50).
 *   fwd: batch statistics of y over (B,D,H,W) -> affine[4][C] = {gamma/std, beta - mean gamma/std,
 *        mean, 1/std}; running statistics updated as nn.BatchNorm3d does (momentum, unbiased var);
 *        out = relu?( y*scale + shift (+ residual) ) on the common corner of y and residual
 *        (relu: 0 none, 1 after the addition, 2 before it).
 *   bwd: dy (B,Dy,Hy,Wy,C), dresidual (B,Dr,Hr,Wr,C) or NULL, both fully written; afterwards
 *        workspace[0..C) = dbeta, workspace[C..2C) = dgamma (doubles).
 * workspace: 2*C doubles.  C % 4 == 0, C <= 256.
 * ------------------------------------------------------------------------- */
typedef struct dsm_bn3d_args {
  const void*  y;             /* conv output (B,Dy,Hy,Wy,C)                          */
  const void*  residual;      /* (B,Dr,Hr,Wr,C) or NULL                              */
  void*        out;           /* (B,Do,Ho,Wo,C), (Do,Ho,Wo) = min(y, residual)       */
  const float* gamma;         /* [C] or NULL (= 1)                                   */
  const float* beta;          /* [C] or NULL (= 0)                                   */
  float*       running_mean;  /* [C] or NULL: updated in fwd                         */
  float*       running_var;   /* [C] or NULL                                         */
  void*        affine;        /* float [4][C]: written by fwd, read by bwd           */
  void*        workspace;     /* double [2][C]                                       */
  const void*  gout;          /* bwd: d loss / d out                                 */
  void*        dy;            /* bwd                                                 */
  void*        dresidual;     /* bwd, or NULL                                        */
  int B, C;
  int Dy, Hy, Wy;
  int Dr, Hr, Wr;
  int relu;
  float momentum, eps;
  /* ABI v6, optional (the fp16 convolution modes' x_amax): max |out| (fwd), max |dy| and
   * max |dresidual| (bwd) are folded into these device floats with an atomic maximum on the float
   * bits; the caller zeroes them first. */
  float*       out_amax;
  float*       dy_amax;
  float*       dres_amax;
} dsm_bn3d_args;
int dsm_bn3d_train_fwd(const dsm_bn3d_args* args, dsm_stream_t stream);
int dsm_bn3d_train_bwd(const dsm_bn3d_args* args, dsm_stream_t stream);

/* NCDHW <-> NDHWC repack of an fp32 volume (used at the boundary with stock
 * torch modules that want contiguous NCDHW). to_ndhwc = 1: src NCDHW. */
int dsm_volume_relayout(const void* src, void* dst, int B, int C, int D, int H, int W,
                        int to_ndhwc, dsm_stream_t stream);

/* PSMNet spatial-pyramid-pooling head on NHWC fp32 maps -- replaces, in eval mode,
 * models/psmnet/submodule.py:81-99 (branch1..4: AvgPool2d(64/32/16/8) -> convbn(128,32,1,1,0,1)
 * -> ReLU; convbn pads the 1x1 convolution by 1, :10-13) and :126-137 (bilinear upsample to the
 * 1/4-resolution grid + concat [raw 64 | skip 128 | branch4 | branch3 | branch2 | branch1]).
 *   dsm_spp_pool8     skip (B,H,W,128) -> p8 (B,H/8,W/8,128), 8x8 means (floor)
 *   dsm_spp_branches  p8 -> four maps, back to back in `branches` (dsm_spp_branch_floats floats):
 *                     map i (i = 0..3 = branch4..branch1) is (B, h8/2^i + 2, w8/2^i + 2, 32);
 *                     w_t [4][128][32] (input-channel major), scale/shift [4][32] = folded BN
 *   dsm_spp_concat    raw (B,H,W,64), skip (B,H,W,128), branches -> out (B,H,W,320)
 * H, W >= 64 (the reference's 64x64 pool needs a full window). */
size_t dsm_spp_branch_floats(int B, int h8, int w8);
int dsm_spp_pool8(const void* skip, void* p8, int B, int H, int W, dsm_stream_t stream);
int dsm_spp_branches(const void* p8, const void* w_t, const void* scale, const void* shift,
                     void* branches, int B, int h8, int w8, dsm_stream_t stream);
int dsm_spp_concat(const void* raw, const void* skip, const void* branches, void* out,
                   int B, int H, int W, float* y_amax /* NULL, or the device scalar raised to max |out| (ABI v7) */,
                   dsm_stream_t stream);

/* Disparity warp, optionally fused with the reconstruction error -- utils/imwrap.py:37-72
 * (imwrap_BCHW with its default arguments) and models/iresnet.py:169-170.
 *   R (B,C,H0,W0), disp (B,1,H,W), out (B,C,H,W), all NCHW fp32;
 *   out = grid_sample(R + delt, grid(disp), bilinear, zeros, align_corners=False)
 *   L (B,C,H,W) non-NULL: out = |L - that|.  delt: the reference's random epsilon, drawn by the
 *   caller (1e-4 * (U[0,1) + 0.1)). */
int dsm_warp_abs_error(const void* L, const void* R, const void* disp, void* out, int B, int C,
                       int H, int W, int H0, int W0, float delt, dsm_stream_t stream);

/* (ABI v7, additive) Backward of dsm_warp_abs_error -- what autograd runs for utils/imwrap.py:37-72
 * (linspace grids, stack, `im_src + delt`, grid_sample) and the sub + abs of models/iresnet.py:169-170.
 * Same sizes and delt as the forward; nothing is saved, v is recomputed from L, R, disp bit for bit.
 *   g (B,C,H,W): the gradient of the forward's out.  L = NULL: the plain warp (gv = g).
 *   gL (B,C,H,W)   = g * sign(L - v)            (sign(0) = 0, as torch.abs)
 *   gR (B,C,H0,W0) += gv * w_tap on every in-bounds tap, gv = -g * sign(L - v): fp32 atomics; zeroed
 *                     by this call on `stream` first (the sum's last bits depend on arrival order)
 *   gdisp (B,1,H,W) = -(W0/(W0-1)) * sum_c gv_c * (wy0 * (ne_c - nw_c) + wy1 * (se_c - sw_c)) with the
 *                     tap values R + delt, 0 out of bounds (ATen's grid_sample backward, zeros padding)
 * Any of gL, gR, gdisp may be NULL: that gradient is skipped.  gL and gdisp are run-to-run identical. */
int dsm_warp_abs_error_bwd(const void* g, const void* L, const void* R, const void* disp,
                           void* gL, void* gR, void* gdisp,
                           int B, int C, int H, int W, int H0, int W0, float delt, dsm_stream_t stream);

/* One decoder level of DispNetC / iResNet (models/dispnetcorr.py:89-132, iresnet.py:119-161,186-193):
 *   out = myCat2d( relu?(up + bias), upsample_x2_bilinear(pr), skip )      (util_fun.py:7-15)
 * up (B,Cu,Hu,Wu): the transposed convolution's output WITHOUT its bias; bias [Cu] or NULL;
 * pr (B,Cp,Hp,Wp) or NULL (Cp = 0); skip (B,Cs,Hs,Ws) or NULL (Cs = 0); all NCHW fp32.
 * out (B, Cu+Cp+Cs, h, w) with h = min(Hu, 2 Hp, Hs), w = min(Wu, 2 Wp, Ws) -- the caller
 * allocates it from those rules.  align_corners = False (what nn.Upsample resolves to today). */
int dsm_decoder_cat(const void* up, const void* bias, const void* pr, const void* skip, void* out,
                    int B, int Cu, int Cp, int Cs, int Hu, int Wu, int Hp, int Wp, int Hs, int Ws,
                    int relu, dsm_stream_t stream);

/* (ABI v7, additive) Backward of dsm_decoder_cat -- what autograd runs for the bias add, the in-place
 * ReLU, nn.Upsample, the three crops and torch.cat of models/dispnetcorr.py:89-132 and
 * iresnet.py:119-161,186-193 (util_fun.py:7-15).  g and out are (B, Cu+Cp+Cs, h, w), h and w as in the
 * forward; out is the forward's result: its first Cu channels carry the ReLU mask (out > 0), needed
 * when relu != 0 only.
 *   g_up (B,Cu,Hu,Wu)   = g[:, :Cu] (times the mask), zero in the cropped-off rows / columns
 *   g_bias [Cu]         = sum of g_up over (b, y, x); one fp32 atomic per block, zeroed by this call
 *   g_pr (B,Cp,Hp,Wp)   = the adjoint of the bilinear x2 upsampling over the h x w crop (gathered)
 *   g_skip (B,Cs,Hs,Ws) = g[:, Cu+Cp:], zero-padded likewise
 * Any of the four may be NULL: that gradient is skipped.  Every element of a requested gradient is
 * written; g_up, g_pr, g_skip have one writer per element.  At most two launches. */
int dsm_decoder_cat_bwd(const void* g, const void* out, void* g_up, void* g_bias, void* g_pr, void* g_skip,
                        int B, int Cu, int Cp, int Cs, int Hu, int Wu, int Hp, int Wp, int Hs, int Ws,
                        int relu, dsm_stream_t stream);

/* (ABI v5) Image staging of the 2-D towers (models/psmnet/stackhourglass.py:118-121 feeds the two
 * views through feature_extraction one after the other; in eval mode they share one batch):
 * left, right (B,C,H,W) NCHW fp32, C <= 16 -> out (2B,16,H,W) in NHWC memory, channels C..15 zero.
 * right = NULL stages one view (B images). */
int dsm_stage_images_nhwc16(const void* left, const void* right, void* out, int B, int C, int H, int W,
                            dsm_stream_t stream);

/* (ABI v7, additive) Self-supervised "depthmono[-mask]" pyramid loss, fused -- losses/loss.py
 * loss_depthmono :196-236, C_ds1 :71-83, weight_common :393-405, losses_pyramid1 :424-467,
 * losses/SSIM.py _ssim :24-42 (11x11 Gaussian, sigma 1.5, zero padding 5, ONE output channel)
 * and utils/imwrap.py:37-72 imwrap_BCHW with LeftTop / scale_factor / fliplr.
 * One item = one (level, side): items 2p and 2p+1 are the two views of one pyramid level and
 *   loss = sum_p (C(item 2p) + C(item 2p+1)) * weight(item 2p).
 * Item: im (B,3,h,w) and src (B,3,H0,W0) fp32 with element strides (b,c,y,x) (pyramid levels are
 * the ::2^k views: no copy); disp, disp_other (B,1,h,w) contiguous; left/top = LeftTop in src
 * pixels; scale_factor = the warp's scale and weight_common's divisor; delt_im / delt_disp = the
 * reference's random epsilons of the image warp and of the (fliplr) disparity warp.
 *   dsm_selfsup_workspace_floats  size of the caller-allocated fp32 workspace (tile partial sums
 *                                 + 5 saved floats per pixel for the backward)
 *   dsm_selfsup_fwd   2 launches (tiles, fixed-order reduction): loss (1 float) and
 *                     aux (4 floats per item: w, fallback flag (< 1024 valid pixels), C, simlary)
 *   dsm_selfsup_bwd   1 launch: ACCUMULATES d loss / d disp into grad_disp and grad_other of
 *                     every item (fp32 global atomics: the left-right terms scatter into the
 *                     other view's disparity); the caller zeroes them.  grad_loss: device scalar.
 * flags: 0 or DSM_SELFSUP_MASK (the "-mask" weights, weight_common) = depthmono, as ever.
 * n_items even, 2..DSM_SELFSUP_MAX_ITEMS.
 *
 * The "Cap[_ds][_lr][-mask]" objective (loss_Cap_ds_lr, loss.py:238-283) on the same entry points:
 * flags = DSM_SELFSUP_CAP | [DSM_SELFSUP_MASK] | [DSM_SELFSUP_DS] | [DSM_SELFSUP_LR].  Its rule:
 * simlary is the mean SSIM over mask_ap however few pixels that is (no fallback: aux slot 1 is 0;
 * no valid pixel at all gives w = 0.001 and an unspecified simlary slot), the smoothness term is
 * weighted w / ds_divisor (ds_divisor 0 means 1; depthmono ignores it), and the smoothness and
 * left-right terms exist only with DS / LR.  Without LR dsm_selfsup_bwd is a pure gather that
 * STORES every element of every item's grad_disp (no atomics, bit-reproducible, the buffers
 * may be uninitialised; grad_other is not touched and may be NULL); without LR and MASK disp_other is never read.
 * With LR it accumulates as above.  Any other flags word is DSM_ERR_ARG. */
#define DSM_SELFSUP_MAX_ITEMS 16
#define DSM_SELFSUP_MASK 1
#define DSM_SELFSUP_CAP 2
#define DSM_SELFSUP_DS 4
#define DSM_SELFSUP_LR 8
typedef struct dsm_selfsup_item {
  const void* im;
  const void* src;
  const void* disp;
  const void* disp_other;
  void* grad_disp;
  void* grad_other;
  int im_stride[4];
  int src_stride[4];
  int B, h, w, H0, W0;
  int left, top, scale_factor;
  float delt_im, delt_disp, weight;
  int ds_divisor; /* Cap: C_ds is weighted w / ds_divisor; 0 = 1 (was padding) */
} dsm_selfsup_item;

size_t dsm_selfsup_workspace_floats(const dsm_selfsup_item* items, int n_items);
int dsm_selfsup_fwd(const dsm_selfsup_item* items, int n_items, int flags, void* workspace,
                    void* loss, void* aux, dsm_stream_t stream);
int dsm_selfsup_bwd(const dsm_selfsup_item* items, int n_items, int flags, const void* workspace,
                    const void* aux, const void* grad_loss, dsm_stream_t stream);

/* (ABI v7, additive) The objectives that the flags word above refuses, on entry points of their
 * own (same items, same aux, same workspace contract with its own size function):
 *   flags = DSM_SELFSUP_COMMON | [DSM_SELFSUP_MASK]   "common[-mask]" (loss_common, loss.py:154-194):
 *     depthmono's rule -- the "< 1024 valid" fallback, both terms, w_ds = w_lr = w -- with the
 *     depth-ratio smoothness C_ds3 (loss.py:99-114) in place of C_ds1.  Forward 3 launches (the
 *     per-sample image-gradient sums in a fixed order, tiles, reduction), backward 1 that
 *     ACCUMULATES as dsm_selfsup_bwd does.  ds_divisor is ignored.
 *     ``ext`` may be NULL.
 *   flags = DSM_SELFSUP_SSSMNET | [DSM_SELFSUP_MASK]  "SsSMnet[-mask]" (loss_SsSMnet, loss.py:285-324,
 *     through losses_pyramid2, :469-512): C_ap with the image-gradient term C_imdiff1, C_lr =
 *     |im - im_wrap1| with im_wrap1 the OTHER view's warped image warped again (fliplr), the
 *     second-order smoothness C_ds2 weighted w / ds_divisor, 1e-4 mean|disp|; w from the mean SSIM
 *     over mask_ap with no fallback (no valid pixel: w = 0.001, aux slot 1 is 0).  ``ext``: one
 *     dsm_selfsup_ext per item -- warp (B,3,h,w) fp32, written by the forward (every item's
 *     im_wrap) and read by the backward; grad_warp (B,3,h,w) fp32, ZEROED by the caller, backward
 *     only; delt_im1, the epsilon of im_wrap1.  delt_disp is read with MASK only, disp_other with
 *     MASK only, grad_other never.  Forward 3 launches (warp, tiles, reduction); backward 2: tiles,
 *     which STORES every element of every grad_disp and scatters d loss / d im_wrap of the other
 *     view into its grad_warp (fp32 atomics), and a chain launch that adds it to grad_disp.
 * Any other flags word is DSM_ERR_ARG; a map with 3 h w >= 2^31 is DSM_ERR_UNSUPPORTED. */
#define DSM_SELFSUP_COMMON 16
#define DSM_SELFSUP_SSSMNET 32
typedef struct dsm_selfsup_ext {
  void* warp;
  void* grad_warp;
  float delt_im1;
  int reserved;
} dsm_selfsup_ext;
size_t dsm_selfsup_ext_workspace_floats(const dsm_selfsup_item* items, int n_items, int flags);
int dsm_selfsup_ext_fwd(const dsm_selfsup_item* items, const dsm_selfsup_ext* ext, int n_items, int flags,
                        void* workspace, void* loss, void* aux, dsm_stream_t stream);
int dsm_selfsup_ext_bwd(const dsm_selfsup_item* items, const dsm_selfsup_ext* ext, int n_items, int flags,
                        const void* workspace, const void* aux, const void* grad_loss, dsm_stream_t stream);

/* (ABI v7, additive) The per-step scalars of the loss from DEVICE memory, so that a captured graph
 * replays with each step's own epsilons and level weights.  `params` is float[n_items][4], 16-byte
 * aligned; row i = {delt_im, delt_disp, delt_im1, weight} of item i (items ordered as above: 2p the
 * left view of entry p, 2p + 1 the flipped one; weight of row 2p is the entry's).  The kernels
 * read it when they RUN, one 16-byte load per workgroup; the items' delt_im / delt_disp / weight
 * and the ext's delt_im1 are ignored.  Both take every flags word of the four entry points above
 * (ext: SsSMnet only, else NULL) and launch the same kernels; workspace sizes as above.
 * params NULL: DSM_ERR_ARG; not 16-byte aligned: DSM_ERR_ALIGN; every other check as above.
 * The array must not change between a forward and its backward. */
int dsm_selfsup_dyn_fwd(const dsm_selfsup_item* items, const dsm_selfsup_ext* ext, int n_items, int flags,
                        const float* params, void* workspace, void* loss, void* aux, dsm_stream_t stream);
int dsm_selfsup_dyn_bwd(const dsm_selfsup_item* items, const dsm_selfsup_ext* ext, int n_items, int flags,
                        const float* params, const void* workspace, const void* aux, const void* grad_loss,
                        dsm_stream_t stream);

/* (ABI v7, additive) Supervised pyramid loss with the D1 / EPE metrics, fused (csrc/suploss.hip) --
 * losses/loss.py loss_supervised :326-338 (diff1_dx / diff1_dy :36-44), losses_pyramid0 :407-421,
 * stereo.py accuracy :103-113.  One item = one weighted output of the model: pred (B,1,hc,wc) fp32
 * contiguous at pyramid level `level` (scale s = 2^level), its weight, and grad (same shape; NULL =
 * no gradient wanted).  gt (B,1,H,W) fp32 contiguous is shared by all items.  Per fine pixel:
 * p = the bilinear sample of F.interpolate(scale_factor=s, align_corners=False) cropped to H x W
 * (the map itself at level 0), m = gt > 0, dx / dy = forward differences of p, zero in the last
 * column / row of the cropped image, sm = min(|dx| + |dy|, 1);  n = sum m over the batch and
 *   loss = sum_items weight * (sum m |gt - p| + 0.1 * flag_smooth * sum m sm) / n    (0 when n == 0).
 *   dsm_suploss_workspace_floats  n_items * (4 * tiles + (save_for_bwd ? B*H*W : 0)) with
 *                     tiles = B * ceil(H/16) * ceil(W/64); 0 for invalid arguments
 *   dsm_suploss_fwd   2 launches (tiles, fixed-order fp64 reduction): loss (1 float) and aux
 *                     (1 + 4 * n_items floats): n, then per item L1 mean, smooth mean, EPE and D1 %
 *                     (good pixel: |gt - p| <= 3 OR |gt - p| / gt <= 0.05; EPE = D1 = NaN when n == 0,
 *                     as accuracy gives).  save_for_bwd: also the unnormalised fine-pixel gradient,
 *                     4 bytes per pixel per item, into the workspace.
 *   dsm_suploss_bwd   1 launch, a gather without atomics (bit-reproducible): OVERWRITES grad of
 *                     every item that has one with d loss / d pred * grad_loss (device scalar);
 *                     the smoothness adjoint passes where |dx| + |dy| <= 1, sign(0) = 0.
 *                     workspace and aux are those of the forward (save_for_bwd != 0).
 * DSM_ERR_ARG (nothing launched): null pointers, n_items outside 1..DSM_SUPLOSS_MAX_ITEMS,
 * non-positive sizes, items of different B.  DSM_ERR_UNSUPPORTED: hc * s < H or wc * s < W
 * (the reference's crop would come out smaller than gt), level > 12, B*H*W >= 2^31.
 * The workspace must be 16-byte aligned (DSM_ERR_ALIGN).  sizeof(dsm_suploss_item) == 48. */
#define DSM_SUPLOSS_MAX_ITEMS 16
typedef struct dsm_suploss_item {
  const void* pred;
  void* grad;
  int B, hc, wc, level;
  float weight;
  int pad_[3];
} dsm_suploss_item;

size_t dsm_suploss_workspace_floats(int n_items, int B, int H, int W, int save_for_bwd);
int dsm_suploss_fwd(const dsm_suploss_item* items, int n_items, const void* gt, int H, int W,
                    int flag_smooth, int save_for_bwd, void* workspace, void* loss, void* aux,
                    dsm_stream_t stream);
int dsm_suploss_bwd(const dsm_suploss_item* items, int n_items, const void* gt, int H, int W,
                    int flag_smooth, const void* workspace, const void* aux, const void* grad_loss,
                    dsm_stream_t stream);

/* (ABI v7, additive) Evaluation metrics of a disparity map, fused (csrc/metrics.hip) -- utils/evaluate.py
 * :9-34 evaluate, :36-44 imwrap_pixel_errors, :46-73 compute_errors, stereo.py:103-113 accuracy.
 * pred (B,1,H,W) fp32 contiguous; gt (B,1,H,W) or NULL; imL and imR (B,C,H,W), both or neither, the same
 * H and W as pred (the warp is utils/imwrap.py:37-72 imwrap_BCHW(imR, +-pred) at LeftTop [0,0], scale 1,
 * with the arithmetic of dsm_warp_abs_error; delt is the reference's random epsilon, drawn by the caller).
 * Two launches (tiles, fixed-order fp64 reduction), no atomics, no host synchronisation: out (B,16) float64
 * gets, per image, with m = gt > 0, diff = |gt - pred| and per-element arithmetic in fp32,
 *    0 count m              1 sum diff          2 count (diff <= 3 or diff/gt <= 0.05)
 *    3 count (diff >= 3 and diff/gt >= 0.05)     4 sum diff^2    5 sum (ln gt - ln(pred + 1e-6))^2
 *    6 sum diff/gt          7 sum diff^2/gt      8-10 count max(gt/(pred + 1e-6), pred/gt) < 1.25, 1.25^2, 1.25^3
 *   11 count, 12 sum |imL - w| over elements with w > 0
 *   13 pixels whose channel sum of w is > 0, 14 sum |imL - w| over all C channels of those pixels
 *   15 sum |imL - w| over every element
 * Slots of an absent input (0-10 without gt, 11-15 without images) are 0.  The rows are additive over
 * images (and over ranks).  workspace: dsm_stereo_metrics_workspace_bytes(B, H, W) bytes =
 * B * ceil(H/16) * ceil(W/64) * 16 * 8 (0 for non-positive sizes), fully overwritten.
 * flags: 0, or DSM_METRICS_NEGATE_WARP (the warp samples at -pred, as evaluate.py:26,40 do).
 * DSM_ERR_ARG (nothing launched): NULL args, pred, out or workspace; imL without imR or the reverse;
 * neither gt nor images; B, C, H or W <= 0 (C = 1 without images); H or W < 2 with images (imwrap.py:48);
 * any other flags word.  DSM_ERR_ALIGN: a map that is not 4-byte aligned, workspace or out not 8-byte
 * aligned.  DSM_ERR_UNSUPPORTED: 2^31 tiles or more.  sizeof(dsm_metrics_args) == 72. */
#define DSM_METRICS_SLOTS 16
#define DSM_METRICS_NEGATE_WARP 1
typedef struct dsm_metrics_args {
  const void* pred;
  const void* gt;
  const void* imL;
  const void* imR;
  void* workspace;
  void* out;
  int B, C, H, W;
  float delt;
  int flags;
} dsm_metrics_args;

size_t dsm_stereo_metrics_workspace_bytes(int B, int H, int W);
int dsm_stereo_metrics(const dsm_metrics_args* args, dsm_stream_t stream);

/* (ABI v7, additive) Left-right consistency check of a disparity map (csrc/lrcheck.hip) -- the warp of
 * utils/imwrap.py:37-72 imwrap_BCHW(other, disp, fliplr=True, LeftTop=[0,0], scale_factor=1) as
 * losses/loss.py:451-452 call it, and the weight of losses/loss.py:393-404 weight_common.
 * disp, other: (B,H,W) fp32 contiguous (a (B,1,H,W) map is the same memory).  One launch, no atomics, no
 * host synchronisation.  Per pixel, in fp32:
 *    wrap    other sampled with grid_sample(bilinear, zeros, align_corners=False) at
 *            x = -(linspace(-1, 1, W)[x] - disp * 2 / (W - 1)), y = linspace(-1, 1, H)[y];
 *            delt (the reference's random epsilon, drawn by the caller; 0 for inference) is added to
 *            the in-bounds taps only
 *    delta   |disp - wrap| / factor
 *    weight  1 for delta < 1, 1 - (delta - 1) * (0.99 / 2) for 1 <= delta < 3, 0.01 from 3 on
 *    mask    uint8, 1 where delta < threshold and the sample position ix = ((gx + 1) * W - 1) / 2 of that x coordinate gx lies in
 *            [0, W - 1] (beyond the reference: a sample half out of the image is no measurement), else 0
 *    masked  disp where mask is set, else 0
 * Each of wrap, weight, mask, masked may be NULL, not all four.
 * flags: 0 -- other is in the mirrored frame (predicted from the mirrored, swapped pair, as dispL1 of
 * loss.py:451) -- or DSM_LRCHECK_OTHER_RIGHT_FRAME: other is the right camera's map in its own frame
 * and is read at column W - 1 - x, without a copy; bit-identical to flags 0 on the mirrored map.
 * DSM_ERR_ARG (nothing launched): NULL args, disp or other; all four outputs NULL; B <= 0; H or W < 2
 * (imwrap.py:48); a factor that is not finite and positive; a threshold that is not finite; any other
 * flags bit.  DSM_ERR_ALIGN: an fp32 map that is not 4-byte aligned.  DSM_ERR_UNSUPPORTED: 2^31 tiles of
 * 16x64 or more.  sizeof(dsm_lrcheck_args) == 80. */
#define DSM_LRCHECK_OTHER_RIGHT_FRAME 1
typedef struct dsm_lrcheck_args {
  const void* disp;
  const void* other;
  void* wrap;
  void* weight;
  void* mask;
  void* masked;
  int B, H, W;
  float delt;
  float factor;
  float threshold;
  int flags;
  int reserved;
} dsm_lrcheck_args;

int dsm_lr_check(const dsm_lrcheck_args* args, dsm_stream_t stream);

/* (ABI v7, additive) Background fill of the pixels a mask rejects (csrc/lrcheck.hip).  disp (B,H,W) fp32,
 * mask (B,H,W) uint8 (non-zero: valid), out (B,H,W) fp32.  Two launches, no atomics, no host
 * synchronisation; the value of an invalid pixel is never read.
 *   rows        a valid pixel is copied; an invalid one gets fminf of the nearest valid pixels to its
 *               left and right in its row, or the one that exists; a row without a valid pixel is empty
 *   empty rows  element by element, fminf of the nearest non-empty rows above and below as filled, or the
 *               one that exists; an image without a valid pixel becomes zeros
 * workspace: dsm_fill_background_workspace_bytes(B, H, W) bytes = B * H * 4 (0 for non-positive sizes),
 * fully overwritten.
 * DSM_ERR_ARG (nothing launched): a NULL pointer; B, H or W <= 0; out overlapping disp, mask or the
 * workspace.  DSM_ERR_ALIGN: disp, out or workspace not 4-byte aligned.  DSM_ERR_UNSUPPORTED: B * H >= 2^31. */
size_t dsm_fill_background_workspace_bytes(int B, int H, int W);
int dsm_fill_background(const void* disp, const void* mask, void* out, void* workspace, int B, int H, int W,
                        dsm_stream_t stream);

/* (ABI v7, additive) Speckle filter of a disparity map (csrc/speckle.hip): the connected regions of the map
 * and the removal of the small ones, OpenCV's filterSpeckles(img, newVal, maxSpeckleSize, maxDiff) on the
 * device.  disp (B,H,W) fp32 contiguous (a (B,1,H,W) map is the same memory); valid (B,H,W) uint8, non-zero =
 * valid, or NULL.  Exact, no tolerance:
 *    node    a pixel whose disp is finite and which valid (if given) allows.  The value of any other pixel
 *            is never used.
 *    edge    two 4-neighbours of one image, both nodes, with fabsf(disp[p] - disp[q]) <= max_diff in fp32.
 *            Images of a batch are never joined.
 *    region  a connected component of that graph (transitive: a ramp of steps <= max_diff is one region).
 *    size    (B,H,W) int32: the number of nodes of the pixel's region, 0 for a pixel that is no node
 *    keep    (B,H,W) uint8: 1 where the pixel is a node and size > max_size, else 0 (a region is a speckle
 *            iff size <= max_size; max_size = 0 removes nothing but the pixels that are no nodes)
 *    out     (B,H,W) fp32: disp where keep, else new_val.  out may be disp itself.
 * Each of out, keep, size may be NULL, not all three.  Three or four launches on `stream` (tile labelling in
 * LDS, union across tile borders, flatten and count, apply), integer atomics only: the results do not depend
 * on the order of execution, two runs give the same bits.  No host synchronisation, capturable, a linear chain.
 * workspace: dsm_speckle_workspace_bytes(B, H, W) bytes = B * H * W * 8 (0 for non-positive sizes): an int32
 * label and an int32 count per pixel, every byte written by the first launch before anything reads it.
 * DSM_ERR_ARG (nothing launched): NULL args, disp or workspace; all three outputs NULL; B, H or W < 1;
 * max_size < 0; max_diff negative, NaN or infinite; flags != 0.  DSM_ERR_ALIGN: disp, out, size or workspace
 * not 4-byte aligned (nothing beyond the types' own alignment is asked for).  DSM_ERR_UNSUPPORTED:
 * B * H * W >= 2^31 (int32 linear indices).  sizeof(dsm_speckle_args) == 80. */
typedef struct dsm_speckle_args {
  const void* disp;
  const void* valid;
  void* out;
  void* keep;
  void* size;
  void* workspace;
  int B, H, W;
  int max_size;
  float max_diff;
  float new_val;
  int flags;
} dsm_speckle_args;

size_t dsm_speckle_workspace_bytes(int B, int H, int W);
int dsm_speckle_filter(const dsm_speckle_args* args, dsm_stream_t stream);

/* (ABI v7, additive) Result maps of a disparity map (csrc/encode.hip), the inverse of dsm_stereo_spatial_raw:
 * from the fp32 map to the bytes of the files a user keeps.  One launch; two with DSM_ENCODE_AUTO_RANGE.  No
 * atomics, no host synchronisation, capturable.
 * Inputs, all in one source frame and read at the same element: disp (B,Hs,Ws) fp32 contiguous (a
 * (B,1,Hs,Ws) map is the same memory); gt (B,Hs,Ws) fp32 or NULL, holes <= 0; mask (B,Hs,Ws) uint8 or NULL,
 * non-zero = valid.
 * Window: output pixel (y, x), 0 <= y < h, 0 <= x < w, reads source pixel (y0 + y, x0 + x) -- how padding
 * added before the forward is cut off.  With DSM_ENCODE_FLIP output column x reads source column
 * x0 + w - 1 - x (a right view predicted from the mirrored, swapped pair): no copy, bit-identical to
 * encoding the flipped tensors.
 * Outputs, dense, each may be NULL, not all four.  d is the prediction, every operation fp32:
 *    u16  (B,h,w) uint16, KITTI's encoding: q = rintf(d * 256.0f) (ties to even) clamped to [1, 65535];
 *         0 where d is not finite or mask is 0.  A finite d <= 0 gives 1: a submission is dense.
 *    u8   (B,h,w) uint8, what stereo.py:174 writes (cv2.imwrite of a float plane = convertTo(CV_8U)):
 *         rintf(d) clamped to [0, 255]; NaN and masked pixels 0, +Inf 255, -Inf 0.
 *    rgb  (B,h,w,3) uint8, viridis (matplotlib's table as bytes, csrc/viridis_lut.hpp):
 *         v = ((d - lo) / (hi - lo)) * 256.0f, entry (int)v; v < 0 gives entry 0, v >= 256 entry 255,
 *         hi == lo entry 0 everywhere (as does a v that is NaN because the range overflows fp32);
 *         non-finite or masked pixels (0,0,0).  lo, hi = vmin, vmax, or with DSM_ENCODE_AUTO_RANGE, per
 *         image, the minimum and maximum over the finite, unmasked pixels inside the window (plt.imsave's
 *         rule; an image without such a pixel is all black).  Auto-range costs one more launch, which writes
 *         per-block extremes to `workspace` (dsm_disp_encode_workspace_bytes(B, h, w) bytes, 0 for
 *         non-positive sizes); the encode launch reduces them itself.
 *    err  (B,h,w,3) uint8, needs gt: the KITTI devkit's log-scale error picture, undilated.  Scored where gt is
 *         finite and > 0 and mask allows it, every other pixel (0,0,0).  e = fabsf(gt - d),
 *         n = fminf(e / 3.0f, (e / gt) / 0.05f); the colour of the bin lo <= n < hi:
 *           [0,1/16) 49,54,149  [1/16,1/8) 69,117,180  [1/8,1/4) 116,173,209  [1/4,1/2) 171,217,233
 *           [1/2,1) 224,243,248  [1,2) 254,224,144  [2,4) 253,174,97  [4,8) 244,109,67  [8,16) 215,48,39
 *           [16,inf) 165,0,38, which a non-finite d on a scored pixel takes too.  The step at n = 1 is D1's.
 * DSM_ERR_ARG (nothing launched): NULL args or disp; all four outputs NULL; err without gt; auto-range rgb
 * without a workspace; a non-positive B, Hs, Ws, h or w; a window that leaves the frame (y0 or x0 < 0,
 * y0 + h > Hs, x0 + w > Ws); with rgb and a fixed range, vmin or vmax not finite or vmax < vmin; any other
 * flags bit; an output (or the workspace in use) overlapping an input, or an output overlapping that workspace.
 * DSM_ERR_ALIGN: disp, gt or the workspace in use not 4-byte aligned, u16 not 2-byte aligned.
 * DSM_ERR_UNSUPPORTED: B * Hs * Ws >= 2^31 (the kernel's 32-bit element indices).
 * sizeof(dsm_encode_args) == 104. */
#define DSM_ENCODE_FLIP 1
#define DSM_ENCODE_AUTO_RANGE 2
typedef struct dsm_encode_args {
  const void* disp;
  const void* gt;
  const void* mask;
  void* u16;
  void* u8;
  void* rgb;
  void* err;
  void* workspace;
  int B, Hs, Ws;
  int y0, x0, h, w;
  float vmin, vmax;
  int flags;
} dsm_encode_args;

size_t dsm_disp_encode_workspace_bytes(int B, int h, int w);
int dsm_disp_encode(const dsm_encode_args* args, dsm_stream_t stream);

/* (ABI v7, additive) Stereo colour augmentation of a training batch, fused -- replaces
 * myTransforms/__init__.py:109-135 Stereo_color / Stereo_normalize applied by Stereo_color_batch,
 * i.e. myTransforms/aug_color.py ColorJitter (RandomOrder :175-203 over Brightness, Contrast,
 * Saturation, Gamma :103-173), Lighting :66-101 and Normalize (ImageNet mean / std) :28-45.
 * x: (B,C,H,W) dense fp32, C >= 6, rewritten IN PLACE; channels 3*groups.. are untouched.
 * One record per (image, group), record b*groups + g for channels 3g..3g+2 of image b, drawn on the
 * host.  Per pixel and group, in this order:
 *   DSM_COLOR_JITTER     the four steps in order[0..3] (0 Brightness x*j[0], 1 Contrast x+j[1],
 *                        2 Saturation x+gray*j[2], 3 Gamma max(x,0)^j[3]), then clamp(0,1);
 *   DSM_COLOR_LIGHTING   x += sum_c eigvec[r][c]*alpha[c]*eigval[c] (ImageNet PCA), clamp(0,1);
 *                        alpha = the 3 floats at alpha + 3*alpha_row (device memory, fp32);
 *   DSM_COLOR_NORMALIZE  (x - mean) / std.
 * j[] holds the scalars as the reference applies them (Brightness / Gamma: 1 + u; Contrast /
 * Saturation: u).  Gamma clamps its base at 0 where the reference yields NaN.
 * groups 1 or 2; n_recs == B*groups; order a permutation of 0..3; alpha_row in [0, B*groups) when
 * LIGHTING is set (alpha may be NULL otherwise).  Records travel in kernel arguments, up to
 * DSM_COLOR_MAX_RECORDS per launch (larger batches: one launch per chunk); no host synchronisation. */
#define DSM_COLOR_JITTER     1
#define DSM_COLOR_LIGHTING   2
#define DSM_COLOR_NORMALIZE  4
#define DSM_COLOR_MAX_RECORDS 64
typedef struct dsm_color_record {
  int order[4];
  float jitter[4];
  int flags;
  int alpha_row;
} dsm_color_record;

int dsm_stereo_color(void* x, const void* alpha, const dsm_color_record* recs, int n_recs, int B, int C,
                     int H, int W, int groups, dsm_stream_t stream);

/* (ABI v7, additive) Stereo spatial augmentation and ToTensor of a training batch, fused -- replaces
 * myTransforms/aug_spatial.py:7-88 Spatial_stereo (random shift of the right view, random crop,
 * optional random scale through cv2.resize, linear) followed by aug_color.py:15-26 ToTensor_numpy.
 *   x  (B, H0, W0, C) fp32 frames, channels last: imL(0:3) | imR(3:6) [| dispL(6) [| dispR(7)]],
 *      6 <= C <= 8; NOT modified (the reference shifts its input in place)
 *   y  (B, C, h, w) dense fp32, fully overwritten
 * One record per image, drawn on the host.  In the frame shifted by `shift` (channels 3..5 and 7
 * read `shift` columns to the right; channels >= 6 get += shift where their value is != 0; width
 * W0 - shift) the source window is [hs, hs + rec.h) x [ws, ws + rec.w).
 *   resize == 0  y = the window, which must be h x w;
 *   resize == 1  y = the window resized to (w, h) by cv2's linear rule: for output column dx,
 *                fx = (float)((dx + 0.5) * scale_x - 0.5) (fp64 inside), sx = floor(fx), fx -= sx;
 *                sx < 0: sx = 0, fx = 0; sx >= rec.w - 1: sx = rec.w - 1, fx = 0; second tap
 *                min(sx + 1, rec.w - 1); rows alike with scale_y, rec.h.  fp32, no contraction:
 *                horizontal S[sx]*(1-fx) + S[sx+1]*fx on both rows, then the same form vertically.
 *                Channels >= 6 are then multiplied by scale_rand.
 * Last, channels < to_tensor_channels (0 or 6) are divided by 255.
 * DSM_ERR_ARG (nothing launched): null pointers, C outside 6..8, n_recs != B, shift outside
 * [0, W0), a window outside [0, W0 - shift) x [0, H0), a resize == 0 window that is not h x w,
 * a scale that is not finite and positive.  DSM_ERR_UNSUPPORTED: one image of x or y with 2^31
 * elements or more.  DSM_ERR_ALIGN: x or y not 4-byte aligned.  Records travel in kernel
 * arguments, up to DSM_SPATIAL_MAX_RECORDS per launch (larger batches: one launch per chunk); no
 * host synchronisation.  sizeof(dsm_spatial_record) == 48. */
#define DSM_SPATIAL_MAX_RECORDS 48
typedef struct dsm_spatial_record {
  int shift;
  int ws, hs, w, h;
  int resize;
  float scale_rand;
  int pad_;
  double scale_x, scale_y;
} dsm_spatial_record;

int dsm_stereo_spatial(const void* x, void* y, const dsm_spatial_record* recs, int n_recs, int B, int C,
                       int H0, int W0, int h, int w, int to_tensor_channels, dsm_stream_t stream);

/* (ABI v7, additive) dsm_stereo_spatial from the decoded files' bytes (csrc/frames.hip, DESIGN.md
 * 13c) -- additionally replaces what myDatasets_stereo/Dataset_stereo.py does on the host in
 * __getitem__: :63-74 Crop_center_bottom, :86-99 np.float32 and the channel concatenation, :121-123
 * the horizontal flip.  The (B, H0, W0, C) fp32 frames are never formed.
 *   raw   raw_bytes bytes on the device holding every sample's planes as decoded:
 *         imL, imR   (Hs, Ws, 3) uint8 RGB, dense, at any byte offset;
 *         dispL/R    (Hs, Ws) per disp_format: DSM_DISP_F32 float32 (a non-finite value reads as
 *                    0, as img_rw.load_gray makes it), DSM_DISP_U16_256 uint16 / 256.0f (KITTI's
 *                    encoding), DSM_DISP_U16 (float)uint16, DSM_DISP_U8 (float)uint8;
 *                    read only for C >= 7 (dispL) and C == 8 (dispR), -1 otherwise
 *   srcs  one per image: frame pixel (y, x, c) is the source pixel at row y0 + y, column
 *         x0 + (flip ? W0 - 1 - x : x) of imL (c < 3), imR (3 <= c < 6), dispL (6), dispR (7).
 *         The flip mirrors every channel and does not swap the views.
 *   y, recs, h, w, to_tensor_channels   as for dsm_stereo_spatial, applied to that frame; the
 *         float sequence is the same, so y is bit-identical to dsm_stereo_spatial on fp32 frames
 *         assembled on the host (uint8 -> float and uint16 / 256 are exact).
 * DSM_ERR_ARG (nothing launched): everything dsm_stereo_spatial refuses for the records; a null
 * pointer; C >= 7 with dispL < 0, C == 8 with dispR < 0; an unknown disp_format; flip not 0 or 1;
 * y0 or x0 negative or a frame that does not fit Hs x Ws; a plane not wholly inside
 * [0, raw_bytes).  DSM_ERR_UNSUPPORTED: one plane, one (fp32) frame or one output image of 2^31
 * bytes or more.  DSM_ERR_ALIGN: y not 4-byte aligned, a uint16 plane at an odd address, a float32
 * plane not 4-byte aligned.  Because every plane is checked against raw_bytes, the kernel cannot
 * read outside raw.  Sources and records travel in kernel arguments, 112 B per image,
 * DSM_FRAMES_MAX_RECORDS per launch (larger batches: one launch per chunk); no host
 * synchronisation.  dsm_stereo_spatial_raw_plan runs the same checks and launches nothing.
 * sizeof(dsm_frame_source) == 64. */
#define DSM_DISP_F32 0
#define DSM_DISP_U16_256 1
#define DSM_DISP_U16 2
#define DSM_DISP_U8 3
#define DSM_FRAMES_MAX_RECORDS 32
typedef struct dsm_frame_source {
  long long imL, imR;     /* byte offsets into raw */
  long long dispL, dispR; /* byte offsets into raw, or -1 */
  int Hs, Ws;             /* this sample's file size (all its planes) */
  int y0, x0;             /* top-left of the H0 x W0 frame inside it */
  int flip;
  int disp_format;
  int pad_[2];
} dsm_frame_source;

int dsm_stereo_spatial_raw(const void* raw, size_t raw_bytes, const dsm_frame_source* srcs, void* y,
                           const dsm_spatial_record* recs, int n_recs, int B, int C, int H0, int W0, int h,
                           int w, int to_tensor_channels, dsm_stream_t stream);
int dsm_stereo_spatial_raw_plan(const void* raw, size_t raw_bytes, const dsm_frame_source* srcs, void* y,
                                const dsm_spatial_record* recs, int n_recs, int B, int C, int H0, int W0,
                                int h, int w, int to_tensor_channels);

/* (ABI v7, additive) First convolution of a concatenation cost volume, from 2-D maps (csrc/sepvol.hip,
 * DESIGN.md 3.2f): y = relu?(conv3d(volume, W; k3 s1 p1) * scale + shift) for the volume of
 * dsm_concat_volume_fwd, which is never formed -- plane d is [left | right shifted by d], so the
 * convolution is F[y, x] + G[y, x - d] of two 2-D images away from the borders, and a sum of 18
 * guarded column-convolution images (KL / KR [dz][dx]) everywhere.  Three launches: the K images
 * (exact fp32-input MFMA), the F / G sums, the broadcast that writes y.  Inference only.
 *   both       (2B, H, W, C) NHWC fp32: the B left maps, then the B right maps; C = 32 or 64
 *              (other multiples of 32: DSM_ERR_UNSUPPORTED -- use dsm_conv3d_fwd with vol_virtual)
 *   w_packed   the (32, 2C, 3,3,3) weight as [side][dz][dx][dy][C/2][2][32 outputs] fp32:
 *              input channel side*C + h*C/2 + cc at [..][cc][h][..]
 *   scale, shift  32 floats each (folded BN), or NULL (1 / 0)
 *   workspace  32*H*(18*B*W + 4*B*(2*W + 2)) floats or more (workspace_floats says how many)
 *   y          (B, D, H, W, 32) NDHWC fp32, fully overwritten
 *   y_amax     NULL, or the device scalar raised to max |y| (atomic max, as dsm_conv3d_args.y_amax)
 *   Cout       must be 32; D, H, W >= 1 (every size works: D < 3 and W < 5 take the general form)
 *   mask_left  nonzero: the left half is zeroed for x < d too (PSMNet); zero: GCNet
 *   flags      0, or tuning: planes per workgroup (default 12) | columns per workgroup << 8 (default 107) |
 *              plain instead of nontemporal stores << 20 */
int dsm_concat_conv_fwd(const void* both, const void* w_packed, const void* scale, const void* shift,
                        void* workspace, size_t workspace_floats, void* y, float* y_amax,
                        int B, int C, int Cout, int D, int H, int W,
                        int mask_left, int relu, int flags, dsm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DSMNET_HIP_H */
