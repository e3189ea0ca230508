"""The per-element error bound of the split-precision convolutions (dsmnet_amd/csrc/split_core.hpp), a CPU
emulation of the split and two faulty variants of it.  No GPU is needed by anything here.

For y = scale * conv(x, w) + shift (+ res), everything in float64 on the CPU:

  aa     = conv(|x|, |w|), the layer's geometry;
  ex, ew = amax_exponent(amax the launch is given), amax_exponent(max |w|): e = 12 - floor(log2 amax), clamped
           to +-60 (the rule of dsm_amax_exponent, restated from its definition -- never read from a kernel);
  floor  = 2^-25 (2^-ex sum |w[co]| + 2^-ew conv(|x|, 1)): an fp16 subnormal term has the absolute step 2^-24 in
           scaled units, so a residual (f16x2) or a value (f16) below fp16's normal range is off by up to half of
           it, per operand element, whatever the element's own size;
  A      = 3 * 2^-22 (f16x2: two operand residuals rounded to 11 bits below an 11-bit hi, and the lo * lo product
           that is never formed), 2^-10 + 2^-22 (f16: two operands rounded to 11 bits), 2^-22 (bf16x3, floor = 0:
           three 8-bit terms and no scaling);
  acc    = c sqrt(n) 2^-24 with c = 2: n fp32 roundings along one output's accumulation (N_ROUNDINGS below); a
           same-sign random walk of round-to-nearest errors reaches ~1.5 sqrt(n) half-ulps at the 4.5 sigma tail
           that 1e5 outputs see, and c = 2 rounds that up;
  bound  = |scale| ((A + acc) aa + floor) + 2^-22 (|scale| aa + |shift| + |res|)   -- ReLU is 1-Lipschitz.

The assertion built on it is max(|y - ref| / bound) <= 1 over all outputs, a bound of 0 demanding err = 0
(``ratio``).  The weight gradients use the same formula with (X, G) in the places of (x, w), the sum running
over voxels; the fused BasicBlock propagates the first layer's bound through the second (``chain_bound``)."""
import math

import torch

MODES = ("f16x2", "f16", "bf16x3")
TERMS = {"f16x2": 3, "f16": 1, "bf16x3": 6}            # MFMA issues per 16-deep product group (mma32)
A_REL = {"f16x2": 3 * 2.0 ** -22, "f16": 2.0 ** -10 + 2.0 ** -22, "bf16x3": 2.0 ** -22}
C_WALK = 2.0
EPILOGUE = 2.0 ** -22


def amax_exponent(amax):
    """e with amax * 2^e in [2^12, 2^13), clamped to +-60; ``amax`` is taken as the float32 it is on the device.
    Zero and float32 subnormals have no exponent field to read: the rule sees 2^-127 and clamps to 60."""
    a = float(torch.tensor(float(amax), dtype=torch.float32).abs())
    if a < 2.0 ** -126:
        return 60
    if math.isinf(a) or math.isnan(a):
        return -60
    m, k = math.frexp(a)                               # a = m 2^k, m in [0.5, 1): floor(log2 a) = k - 1
    return max(-60, min(60, 12 - (k - 1)))


# n, the fp32 roundings on the longest accumulation chain of one output, per kernel family.  K: products that can
# be non-zero for one output (taps x input channels; a transposed layer's outputs see at most 2 per axis of its 3
# taps, the other MFMA issues add exact zeros); one MFMA issue = one rounding of the accumulator per term.
#   conv_split.hpp, conv_zs.hpp, deconv_zs.hpp, basicblock2d.hpp (each of its two layers): one accumulator per
#       output walks every (chunk, tap) -> terms * ceil(K / 16);
#   conv_wide2d.hpp (3x3, transposed, 5x5): the same inside a K-range, then wide2d_reduce_kernel adds the KS
#       ranges' partial sums in index order -> + (KS - 1), KS read from the plan's name;
#   conv3d_bwd.hip wgrad_split_kernel: K = voxels; every 32 x TY tile of G is walked in 16-voxel groups (2 TY per
#       tile, padded tiles included), the workgroups' sums meet in one float atomic each, and the 2-D form first
#       folds its four waves' sums (3 additions) -> terms * tiles * 2 TY + workgroups * (1 | 4).
def n_forward(mode, K, ksplit=1):
    return TERMS[mode] * int(math.ceil(K / 16.0)) + (ksplit - 1)


def n_wgrad(mode, tiles, TY, workgroups, two_d):
    return TERMS[mode] * tiles * 2 * TY + workgroups * (4 if two_d else 1)


N_ROUNDINGS = {
    "conv_split": n_forward, "conv_zs": n_forward, "deconv_zs": n_forward, "basicblock2d": n_forward,
    "wide": n_forward, "wide_transposed": n_forward, "k5": n_forward,
    "conv3d_wgrad": n_wgrad, "conv2d_wgrad": n_wgrad,
}


def _bc(v, like, axis=1):
    """A per-channel vector shaped to broadcast over ``like`` along ``axis``; None stays None."""
    if v is None:
        return None
    shape = [1] * like.dim()
    shape[axis] = -1
    return v.double().reshape(shape)


def conv_terms(x, w, conv, cout_axis=0, out_axis=1):
    """The three float64 convolutions a case needs: ``pre`` = conv(x, w), ``aa`` = conv(|x|, |w|), ``ax`` =
    conv(|x|, 1), and ``wsum`` = sum |w[co]| shaped like the channel axis of the output.  ``conv``: the layer's
    geometry as a function of (input, weight) in float64; ``cout_axis``: where the weight keeps Cout;
    ``out_axis``: where the output does (0 for a weight gradient)."""
    x, w = x.double(), w.double()
    pre = conv(x, w)
    aa = conv(x.abs(), w.abs())
    ax = conv(x.abs(), torch.ones_like(w))
    other = [d for d in range(w.dim()) if d != cout_axis]
    wsum = _bc(w.abs().sum(dim=other), pre, out_axis)
    return {"pre": pre, "aa": aa, "ax": ax, "wsum": wsum}


def bound_from_terms(t, mode, n, x_amax, w_amax, scale=None, shift=None, res=None, extra=None):
    """(ref, bound) before the activation.  ``scale`` / ``shift``: per output channel or None; ``res``: already
    cropped to the output (the terms too: ``crop``); ``extra``: an error already present in conv's output
    (unscaled), added under |scale| -- the propagated term of a fused pair."""
    pre, aa = t["pre"], t["aa"]
    sc = _bc(scale, pre) if scale is not None else torch.ones(1, dtype=torch.float64)
    sh = _bc(shift, pre) if shift is not None else torch.zeros(1, dtype=torch.float64)
    rs = res.double() if res is not None else torch.zeros(1, dtype=torch.float64)
    if mode == "bf16x3":
        floor = torch.zeros(1, dtype=torch.float64)
    else:
        ex, ew = amax_exponent(x_amax), amax_exponent(w_amax)
        floor = 2.0 ** -25 * (2.0 ** -ex * t["wsum"] + 2.0 ** -ew * t["ax"])
    acc = C_WALK * math.sqrt(n) * 2.0 ** -24
    inner = (A_REL[mode] + acc) * aa + floor
    if extra is not None:
        inner = inner + extra
    bound = sc.abs() * inner + EPILOGUE * (sc.abs() * aa + sh.abs() + rs.abs())
    return pre * sc + sh + rs, bound.expand_as(pre)


def crop(t, size):
    """The terms cut to the corner ``size`` of the output (a skip shorter than the layer's natural output)."""
    idx = (slice(None), slice(None)) + tuple(slice(0, s) for s in size)
    return {k: (v[idx] if k != "wsum" else v) for k, v in t.items()}


def ratio(y, ref, bound):
    """max |y - ref| / bound over all outputs; an output whose bound is 0 must be exact (else inf)."""
    err = (y.detach().double().cpu() - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf),
                                                                       torch.zeros_like(err)))
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return r.max().item()


def chain_bound(x, w1, w2, conv, mode, n1, n2, x_amax, scale1, shift1, scale2, shift2, res=None):
    """(ref, bound) before the last activation of conv2(relu(conv1(x) s1 + h1)) s2 + h2 (+ res): E1 = the first
    layer's bound on the intermediate h; the second layer multiplies what the kernel really holds, at most
    relu(h) + E1 per element, scaled by a maximum that is at most max relu(h) + max E1 (the kernel takes each
    tile's own, which is no larger: a smaller maximum only lowers the floor); E1 itself passes through |w2|."""
    t1 = conv_terms(x, w1, conv)
    h, e1 = bound_from_terms(t1, mode, n1, x_amax, w1.abs().max().item(), scale1, shift1)
    hr = h.relu()
    t2 = conv_terms(hr, w2, conv)
    grown = conv_terms(hr + e1, w2, conv)                # |operand| the kernel may hold: for aa and conv(|x|, 1)
    t2["aa"], t2["ax"] = grown["aa"], grown["ax"]
    through = conv(e1, w2.double().abs())
    return bound_from_terms(t2, mode, n2, (hr + e1).max().item(), w2.abs().max().item(), scale2, shift2, res,
                            extra=through)


# ------------------------------------------------------------------------------------ the emulated split --
def _split(v, e, mode, mutant):
    """The 16-bit terms of the float32 tensor ``v`` scaled by 2^e, as float64 tensors (split_pair)."""
    if mode == "bf16x3":
        terms, r = [], v.float()
        for _ in range(3):
            t = r.bfloat16().float()
            terms.append(t.double())
            r = r - t
        return terms
    s = v.float() * float(2.0 ** e)                      # exact: a power of two
    hi = s.half()                                        # Tensor.half() rounds to nearest even and keeps subnormals
    if mode == "f16":
        return [hi.double()]
    lo = (s - hi.float()).half()                         # the residual is exact in fp32, then rounded once
    if mutant == "drop_lo":
        lo = torch.zeros_like(lo)
    elif mutant == "flush_lo":
        lo = torch.where(lo.float().abs() < 2.0 ** -14, torch.zeros_like(lo), lo)
    elif mutant is not None:
        raise ValueError(mutant)
    return [hi.double(), lo.double()]


def emulate(x, w, conv, mode, x_amax=None, mutant=None):
    """conv(x, w) as the split kernels form it, products and sums in float64: the operand terms of ``_split``, the
    product groups of mma32 (f16x2: wl xh + wh xl + wh xh; bf16x3: the six with the smallest dropped), the factor
    2^-(ex + ew) taken off at the end.  ``mutant``: None, "drop_lo" (the low term lost: f16x2 degrades to f16) or
    "flush_lo" (residuals below fp16's normal range flushed to zero)."""
    ex = ew = 0
    if mode != "bf16x3":
        ex = amax_exponent(x.abs().max().item() if x_amax is None else x_amax)
        ew = amax_exponent(w.abs().max().item())
    xs, ws = _split(x, ex, mode, mutant), _split(w, ew, mode, mutant)
    pairs = {"f16x2": [(1, 0), (0, 1), (0, 0)], "f16": [(0, 0)],
             "bf16x3": [(1, 1), (2, 0), (0, 2), (1, 0), (0, 1), (0, 0)]}[mode]
    y = None
    for iw, ix in pairs:
        p = conv(xs[ix], ws[iw])
        y = p if y is None else y + p
    return y * 2.0 ** -(ex + ew)


# ------------------------------------------------------------------------------------- the input classes --
CLASSES = ("G", "O4", "O6", "Q", "L", "C", "Z", "Wt")
HEAVY = ("O4", "O6", "Q", "L")


def relu_like(seed, *shape, scale=1.0):
    """The base of every class: tests/test_f16_gpu.py::relu_like (a seeded Gaussian with 30 % zeros)."""
    from tests.test_f16_gpu import relu_like as base
    return base(seed, *shape, scale=scale)


def _loud(v, factor):
    """``v`` x ``factor``, ``v`` first raised to the Gaussian's unit size where the draw (or its ReLU zero) is
    smaller: the outlier then stands at least ``factor`` above the bulk whatever the seed."""
    return math.copysign(max(abs(v), 1.0), v if v != 0 else 1.0) * factor


def make_input(cls, seed, shape, w=None):
    """(x, w) of class ``cls`` on the ``relu_like`` base; ``shape`` = (B, C, spatial...); the last axis is the
    one that tiles are ragged along.  ``w`` comes back untouched except in class Wt."""
    x = relu_like(seed, *shape)
    mid = tuple(s // 2 for s in shape)
    last = (shape[0] - 1, shape[1] // 2) + tuple(s - 1 for s in shape[2:])
    if cls == "G" or cls == "Wt":
        pass
    elif cls == "O4":                                    # one element x 1e4, interior
        x[mid] = _loud(x[mid].item(), 1e4)
    elif cls == "O6":                                    # one element x 1e6, in the last ragged tile
        x[last] = _loud(x[last].item(), 1e6)
    elif cls == "Q":                                     # half the columns quiet, 2^-18 below the rest
        half = shape[-1] // 2
        x[..., :half] *= 2.0 ** -12
        x[..., half:] *= 2.0 ** 6
    elif cls == "L":                                     # sign * exp(3 |n|): log-normal magnitudes
        x = torch.sign(x) * torch.exp(3.0 * x.abs())
    elif cls == "C":                                     # one input channel x 2^12
        x[:, shape[1] // 3] *= 2.0 ** 12
    elif cls == "Z":                                     # all zero but one element
        v = _loud(x[mid].item(), 1.0)
        x = torch.zeros_like(x)
        x[mid] = v
    else:
        raise ValueError(cls)
    if cls == "Wt" and w is not None:                    # one tap of one output channel x 1e3
        w = w.clone()
        tap = tuple(s - 1 if i else 0 for i, s in enumerate(w.shape[2:]))
        w[(w.shape[0] // 2, slice(None)) + tap] *= 1e3
    return x, w


def with_max(x, target):
    """``x`` rescaled by a power of two and its largest element set so that max |x| is exactly ``target``."""
    a = x.abs().max().item()
    k = math.floor(math.log2(target / a))
    y = x.double() * 2.0 ** k
    while y.abs().max().item() >= target:
        y = y * 0.5
    i = y.abs().argmax()
    flat = y.reshape(-1).clone()
    flat[i] = math.copysign(target, flat[i].item())
    return flat.reshape(x.shape).float()
