"""Stereo cost-volume ops of the DSMnet path as ``torch.autograd.Function``s.

Every op is a thin host wrapper over the C ABI of ``include/dsmnet_hip.h``
(``libdsmnet_hip.so``, hand-written HIP for gfx950), launched on PyTorch's
current HIP stream.  PyTorch is plumbing here: device memory, streams, autograd
book-keeping.  There is no CPU path -- CPU tensors raise.

Reference code each op replaces (sunshinnnn/DSMnet):
  corr1d          models/util_conv.py:56-86           (Corr1d)
  concat_volume   models/gcnet.py:130-135, models/psmnet/stackhourglass.py:124-133
  soft_argmin     models/psmnet/stackhourglass.py:152-166 + submodule.py:56-63,
                  models/gcnet.py:104-111
  conv3d_block    models/psmnet/submodule.py:16-19, stackhourglass.py:22-62,
                  models/util_conv.py:150-179, models/util_fun.py:41-50
  stereo_color    myTransforms/aug_color.py:28-45, 66-101, 103-203, myTransforms/__init__.py:109-135
  supervised_pyramid_loss   losses/loss.py:326-338, 407-421, stereo.py:103-113
  stereo_metrics  utils/evaluate.py:9-73, stereo.py:103-113, utils/imwrap.py:37-72
  lr_check        utils/imwrap.py:37-72 (fliplr=True), losses/loss.py:393-404, 451-452
  filter_speckles  beyond the reference: OpenCV's filterSpeckles (connected regions, the small ones removed)
  soft_argmin_confidence   the softmax of the two soft_argmin sites above, kept for its peak, window and entropy
"""
import collections
import ctypes
import functools
import os
import weakref

import torch

from . import _lib
from .folds import _versions

_CL3D = torch.channels_last_3d


class LaunchTimer(object):
    """Per-launch timing with HIP events recorded on the launch stream (the stream the
    kernels are enqueued on -- PyTorch's current stream).  Install with ``set_timer``;
    bench.py reads ``summary()`` after a synchronise.  Costs two event records per launch."""

    def __init__(self):
        self.records = []

    def start(self):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def stop(self, name, start, work):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        self.records.append((name, start, ev, work))

    def summary(self):
        """name -> dict(launches, ms, work); ``work`` is the algorithmic bytes (HBM-bound
        kernels) or FLOPs (MFMA kernels) summed over the launches.  Call after a sync."""
        out = {}
        for name, a, b, work in self.records:
            e = out.setdefault(name, {"launches": 0, "ms": 0.0, "work": 0.0})
            e["launches"] += 1
            e["ms"] += a.elapsed_time(b)
            e["work"] += work
        return out


_timer = None


def set_timer(timer):
    global _timer
    _timer = timer


class _timed(object):
    """``work``: algorithmic bytes or FLOPs of the launch (SURVEY.md section 8d counting)."""

    def __init__(self, name, work=0.0):
        self.name, self.work = name, work

    def __enter__(self):
        self.t0 = _timer.start() if _timer is not None else None

    def __exit__(self, *exc):
        if self.t0 is not None:
            _timer.stop(self.name() if callable(self.name) else self.name, self.t0, self.work)
        return False


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _plan_name(fn, *args):
    """Branch name written by one of the host-only ``dsm_*_plan`` queries (include/dsmnet_hip.h).  Pointer
    arguments are tensors, raw addresses or None: only NULL-ness and 16-byte alignment are looked at, so
    this needs no GPU.  An argument struct goes by reference.  Raises what the launch itself would be refused
    with."""
    buf = ctypes.create_string_buffer(96)
    conv = [_p(a) if isinstance(a, torch.Tensor) else ctypes.byref(a) if isinstance(a, ctypes.Structure) else a
            for a in args]
    _lib.check(getattr(_lib.load(), fn)(*(conv + [buf, 96])), fn)
    return buf.value.decode()


def corr1d_plan_name(fL, fR, out, tmp, B, C, H, W, D, stride=1, kernel_size=1):
    """Kernel(s) ``dsm_corr1d_fwd`` picks (``dsm_corr1d_plan``): ``tile<S,NDH>``, ``fwd<S>vec``,
    ``fwd<S>scalar`` or ``generic``, with ``+box3`` / ``+box`` when a box filter follows."""
    return _plan_name("dsm_corr1d_plan", fL, fR, out, tmp, B, C, H, W, D, stride, kernel_size, _lib.DSM_F32)


def concat_volume_plan_name(fL, fR, vol, B, C, H, W, D, mask_left, channels_last=True, backward=False):
    """Kernel ``dsm_concat_volume_fwd`` (``_bwd``: pass gvol, dfL, dfR) picks: ``ndhwc``,
    ``ndhwc lds>64K``, ``ncdhw vec``, ``ncdhw scalar``; ``ndhwc_bwd``, ``ncdhw_bwd``."""
    return _plan_name("dsm_concat_volume_bwd_plan" if backward else "dsm_concat_volume_fwd_plan", fL, fR, vol,
                      B, C, H, W, D, int(mask_left), _lib.DSM_NDHWC if channels_last else _lib.DSM_NCDHW,
                      _lib.DSM_F32)


def soft_argmin_fwd_plan_name(cost, disp, stats, B, Dc, Hc, Wc, D, H, W, negate=False, align_corners=False):
    """Kernel ``dsm_soft_argmin_fwd`` picks: ``up4<4>``, ``fwd<true,DS>`` or ``fwd<false,DS>``."""
    return _plan_name("dsm_soft_argmin_fwd_plan", cost, disp, stats, B, Dc, Hc, Wc, D, H, W, int(negate),
                      int(align_corners), _lib.DSM_F32)


def soft_argmin_bwd_plan_name(cost, disp, stats, gdisp, dcost, B, Dc, Hc, Wc, D, H, W, negate=False,
                              align_corners=False):
    """Kernel ``dsm_soft_argmin_bwd`` picks: ``bwd_direct``, ``bwd_tile nseg=N`` or ``bwd_fallback``."""
    return _plan_name("dsm_soft_argmin_bwd_plan", cost, disp, stats, gdisp, dcost, B, Dc, Hc, Wc, D, H, W,
                      int(negate), int(align_corners), _lib.DSM_F32)


def confidence_plan_name(cost, disp, B, Dc, Hc, Wc, D, H, W, negate=False, align_corners=False, radius=4):
    """Kernel ``dsm_disp_confidence_fwd`` picks: ``conf_up4<4>``, ``conf<true,DS>`` or ``conf<false,DS>``."""
    return _plan_name("dsm_disp_confidence_fwd_plan", cost, disp, None, None, None, None, B, Dc, Hc, Wc, D, H, W,
                      int(negate), int(align_corners), int(radius), _lib.DSM_F32)


def _require_device(name, *tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "%s: dsmnet_amd ops run on the MI355X through libdsmnet_hip.so only; got a %s "
                "tensor (there is no CPU fallback)" % (name, t.device.type))
        if t.dtype != torch.float32:
            raise TypeError("%s: only float32 is implemented, got %s" % (name, t.dtype))


def _same_shape(name, a, b):
    if a.shape != b.shape:
        # the reference asserts this in its model forwards (gcnet.py:127, dispnetcorr.py:67)
        raise ValueError("%s: left/right feature shapes differ: %s vs %s"
                         % (name, tuple(a.shape), tuple(b.shape)))


# ----------------------------------------------------------------------------
# (a1) Corr1d
# ----------------------------------------------------------------------------
class Corr1dFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fL, fR, D, stride, kernel_size):
        _require_device("corr1d", fL, fR)
        if fL.dim() != 4:
            raise ValueError("corr1d: expected (B,C,H,W) features, got %d-D" % fL.dim())
        _same_shape("corr1d", fL, fR)
        if kernel_size % 2 != 1:
            raise AssertionError("kernel_size must be odd")      # util_conv.py:83
        fL, fR = fL.contiguous(), fR.contiguous()
        B, C, H, W = fL.shape
        out = torch.empty((B, D, H, W), device=fL.device, dtype=fL.dtype)
        tmp = torch.empty_like(out) if kernel_size > 1 else None
        lib = _lib.load()
        with torch.cuda.device(fL.device), _timed("corr1d_fwd_kernel", 4.0 * (2 * B * C * H * W + B * D * H * W)):
            rc = lib.dsm_corr1d_fwd(_p(fL), _p(fR), _p(out), _p(tmp), B, C, H, W, D, stride,
                                    kernel_size, _lib.DSM_F32, _stream())
        _lib.check(rc, "dsm_corr1d_fwd")
        ctx.save_for_backward(fL, fR)
        ctx.cfg = (D, stride, kernel_size)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        fL, fR = ctx.saved_tensors
        D, stride, kernel_size = ctx.cfg
        g = grad_out.contiguous()
        B, C, H, W = fL.shape
        if _OPTIONS["corr1d_tiled_bwd"]:
            dfL, dfR = _corr1d_sim_bwd(g, fL, fR, None, None, D, stride, kernel_size, _lib.DSM_SIM_DOT, 0.0)
            return dfL, dfR, None, None, None
        dfL, dfR = torch.empty_like(fL), torch.empty_like(fR)
        tmp = torch.empty_like(g) if kernel_size > 1 else None
        lib = _lib.load()
        with torch.cuda.device(fL.device):
            rc = lib.dsm_corr1d_bwd(_p(g), _p(fL), _p(fR), _p(dfL), _p(dfR), _p(tmp), B, C, H, W,
                                    D, stride, kernel_size, _lib.DSM_F32, _stream())
        _lib.check(rc, "dsm_corr1d_bwd")
        return dfL, dfR, None, None, None


_SIMS = {"dot": _lib.DSM_SIM_DOT, "cosine": _lib.DSM_SIM_COSINE}


def corr1d_sim_fwd_plan_name(fL, fR, out, raw, inv, B, C, H, W, D, stride=1, kernel_size=1, sim="cosine", eps=1e-8):
    """Kernels ``dsm_corr1d_sim_fwd`` picks (``dsm_corr1d_sim_fwd_plan``): the names of ``corr1d_plan_name``,
    with the prefix ``cos:`` for the cosine similarity."""
    return _plan_name("dsm_corr1d_sim_fwd_plan", fL, fR, out, raw, inv, B, C, H, W, D, stride, kernel_size,
                      _SIMS[sim], ctypes.c_float(eps), _lib.DSM_F32)


def corr1d_sim_bwd_plan_name(grad_out, fL, fR, raw, inv, dfL, dfR, workspace, B, C, H, W, D, stride=1,
                             kernel_size=1, sim="cosine", eps=1e-8, flags=0):
    """Kernels ``dsm_corr1d_sim_bwd`` picks (``dsm_corr1d_sim_bwd_plan``): ``bwd_tile<S>`` or ``bwd_naive``,
    behind ``prep+`` (cosine) and ``box3+`` / ``box+`` (kernel_size > 1)."""
    return _plan_name("dsm_corr1d_sim_bwd_plan", grad_out, fL, fR, raw, inv, dfL, dfR, workspace, B, C, H, W, D,
                      stride, kernel_size, _SIMS[sim], ctypes.c_float(eps), int(flags), _lib.DSM_F32)


def _corr1d_sim_bwd(g, fL, fR, raw, inv, D, stride, kernel_size, sim, eps, flags=0):
    """``dsm_corr1d_sim_bwd``: the tiled data gradient wherever its plan admits it (``flags``: DSM_CORR_BWD_NAIVE
    forces the naive kernel).  No host read, no synchronisation."""
    B, C, H, W = fL.shape
    lib = _lib.load()
    dfL, dfR = torch.empty_like(fL), torch.empty_like(fR)
    nbytes = lib.dsm_corr1d_sim_workspace_bytes(B, C, H, W, D, kernel_size, sim)
    ws = torch.empty(nbytes // 4, device=fL.device, dtype=torch.float32) if nbytes else None
    with torch.cuda.device(fL.device), _timed("corr1d_bwd_kernel", 4.0 * (4 * B * C * H * W + B * D * H * W)):
        rc = lib.dsm_corr1d_sim_bwd(_p(g), _p(fL), _p(fR), _p(raw), _p(inv), _p(dfL), _p(dfR), _p(ws), B, C, H, W,
                                    D, stride, kernel_size, sim, eps, flags, _lib.DSM_F32, _stream())
    _lib.check(rc, "dsm_corr1d_sim_bwd")
    return dfL, dfR


class Corr1dCosineFunction(torch.autograd.Function):
    """``Corr1d(simfun=nn.CosineSimilarity(dim=1, eps))``: ``dsm_corr1d_sim_fwd`` / ``_bwd`` with DSM_SIM_COSINE
    (include/dsmnet_hip.h has the formula and its gradients).  Saves the features, the inverse norms and the raw
    (unfiltered) map; capturable in a graph."""

    @staticmethod
    def forward(ctx, fL, fR, D, stride, kernel_size, eps):
        _require_device("corr1d", fL, fR)
        if fL.dim() != 4:
            raise ValueError("corr1d: expected (B,C,H,W) features, got %d-D" % fL.dim())
        _same_shape("corr1d", fL, fR)
        if kernel_size % 2 != 1:
            raise AssertionError("kernel_size must be odd")      # util_conv.py:83
        fL, fR = fL.contiguous(), fR.contiguous()
        B, C, H, W = fL.shape
        out = torch.empty((B, D, H, W), device=fL.device, dtype=fL.dtype)
        raw = torch.empty_like(out) if kernel_size > 1 else None
        inv = torch.empty((2, B, H, W), device=fL.device, dtype=fL.dtype)
        lib = _lib.load()
        with torch.cuda.device(fL.device), _timed("corr1d_cosine_fwd_kernel", 4.0 * (4 * B * C * H * W + B * D * H * W)):
            rc = lib.dsm_corr1d_sim_fwd(_p(fL), _p(fR), _p(out), _p(raw), _p(inv), B, C, H, W, D, stride,
                                        kernel_size, _lib.DSM_SIM_COSINE, eps, _lib.DSM_F32, _stream())
        _lib.check(rc, "dsm_corr1d_sim_fwd")
        ctx.save_for_backward(fL, fR, inv, out if raw is None else raw)
        ctx.cfg = (D, stride, kernel_size, eps)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        fL, fR, inv, raw = ctx.saved_tensors
        D, stride, kernel_size, eps = ctx.cfg
        dfL, dfR = _corr1d_sim_bwd(grad_out.contiguous(), fL, fR, raw, inv, D, stride, kernel_size,
                                   _lib.DSM_SIM_COSINE, eps)
        return dfL, dfR, None, None, None, None


def corr1d(fL, fR, D, stride=1, kernel_size=1, sim="dot", eps=1e-8):
    """``Corr1d(kernel_size, stride, D, simfun).forward(fL, fR)`` -> (B, D, H, W).  ``sim``: "dot" (the
    reference's default similarity) or "cosine" (``nn.CosineSimilarity(dim=1, eps)``: each norm clamped at
    ``eps`` on its own, a clamped norm constant in the gradient)."""
    if sim == "dot":
        return Corr1dFunction.apply(fL, fR, int(D), int(stride), int(kernel_size))
    if sim != "cosine":
        raise ValueError("corr1d: sim must be 'dot' or 'cosine', got %r" % (sim,))
    return Corr1dCosineFunction.apply(fL, fR, int(D), int(stride), int(kernel_size), float(eps))


# ----------------------------------------------------------------------------
# (a2, a3) concatenation cost volume
# ----------------------------------------------------------------------------
def concat_volume_right(fL, fR, D):
    """The right-referenced volume of ``gcnet_LR`` (models/gcnet.py:155-164), (B, 2C, D, H, W)
    channels_last_3d: right features at every x, ``vol[:, C:, d, y, x] = fL[y, x + d]`` for
    ``x + d < W``.  Same kernel as ``concat_volume`` walking the other way.  Inference only."""
    _require_device("concat_volume_right", fL, fR)
    _same_shape("concat_volume_right", fL, fR)
    if fL.requires_grad or fR.requires_grad:
        if torch.is_grad_enabled():
            raise NotImplementedError("concat_volume_right has no backward (gcnet_LR is not reachable "
                                      "from the reference's model factory)")
    fL, fR = fL.contiguous(), fR.contiguous()
    B, C, H, W = fL.shape
    vol = torch.empty((B, 2 * C, D, H, W), device=fL.device, dtype=fL.dtype, memory_format=_CL3D)
    with torch.cuda.device(fL.device), _timed("volume_ndhwc_fwd_kernel", 4.0 * (2 * B * C * H * W + 2 * B * C * D * H * W)):
        rc = _lib.load().dsm_concat_volume_fwd(_p(fR), _p(fL), _p(vol), B, C, H, W, int(D), 2,
                                               _lib.DSM_NDHWC, _lib.DSM_F32, _stream())
    _lib.check(rc, "dsm_concat_volume_fwd")
    return vol


class ConcatVolumeFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fL, fR, D, mask_left, channels_last):
        _require_device("concat_volume", fL, fR)
        if fL.dim() != 4:
            raise ValueError("concat_volume: expected (B,C,H,W) features, got %d-D" % fL.dim())
        _same_shape("concat_volume", fL, fR)
        fL, fR = fL.contiguous(), fR.contiguous()
        B, C, H, W = fL.shape
        fmt = _CL3D if channels_last else torch.contiguous_format
        vol = torch.empty((B, 2 * C, D, H, W), device=fL.device, dtype=fL.dtype,
                          memory_format=fmt)
        layout = _lib.DSM_NDHWC if channels_last else _lib.DSM_NCDHW
        lib = _lib.load()
        with torch.cuda.device(fL.device), \
                _timed("volume_ndhwc_fwd_kernel" if channels_last else "volume_ncdhw_fwd_kernel",
                       4.0 * (2 * B * C * H * W + 2 * B * C * D * H * W)):
            rc = lib.dsm_concat_volume_fwd(_p(fL), _p(fR), _p(vol), B, C, H, W, D,
                                           int(mask_left), layout, _lib.DSM_F32, _stream())
        _lib.check(rc, "dsm_concat_volume_fwd")
        ctx.cfg = (B, C, H, W, D, int(mask_left), layout, fmt)
        return vol

    @staticmethod
    def backward(ctx, gvol):
        B, C, H, W, D, mask_left, layout, fmt = ctx.cfg
        g = gvol.contiguous(memory_format=fmt)
        dfL = torch.empty((B, C, H, W), device=g.device, dtype=g.dtype)
        dfR = torch.empty_like(dfL)
        lib = _lib.load()
        with torch.cuda.device(g.device):
            rc = lib.dsm_concat_volume_bwd(_p(g), _p(dfL), _p(dfR), B, C, H, W, D, mask_left,
                                           layout, _lib.DSM_F32, _stream())
        _lib.check(rc, "dsm_concat_volume_bwd")
        return dfL, dfR, None, None, None


def concat_volume(fL, fR, D, mask_left, channels_last=True):
    """Concatenation cost volume (B, 2C, D, H, W).

    ``mask_left=False``: GCNet (gcnet.py:130-135); ``True``: PSMNet
    (stackhourglass.py:124-133).  ``channels_last`` selects the memory format of the
    result: ``torch.channels_last_3d`` (what ``conv3d_block`` consumes) or contiguous."""
    vol = ConcatVolumeFunction.apply(fL, fR, int(D), bool(mask_left), bool(channels_last))
    sl = getattr(fL, "_dsm_amax", None)
    if sl is not None and sl is getattr(fR, "_dsm_amax", None):
        vol._dsm_amax = sl                  # copies of the features: the same bound holds
    return vol


# ----------------------------------------------------------------------------
# (a6, a7) soft-argmin
# ----------------------------------------------------------------------------
class SoftArgminFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cost, out_size, negate, align_corners):
        _require_device("soft_argmin", cost)
        if cost.dim() == 5:
            if cost.shape[1] != 1:
                raise ValueError("soft_argmin: 5-D cost must have one channel")
            c4 = cost.reshape(cost.shape[0], *cost.shape[2:])
        elif cost.dim() == 4:
            c4 = cost
        else:
            raise ValueError("soft_argmin: expected (B,1,D,H,W) or (B,D,H,W)")
        c4 = c4.contiguous()
        B, Dc, Hc, Wc = c4.shape
        D, H, W = (Dc, Hc, Wc) if out_size is None else tuple(int(v) for v in out_size)
        disp = torch.empty((B, H, W), device=cost.device, dtype=cost.dtype)
        need_grad = ctx.needs_input_grad[0]
        stats = torch.empty((B, 2, H, W), device=cost.device, dtype=cost.dtype) if need_grad else None
        lib = _lib.load()
        # the x4 fast path (soft_argmin.hip: dsm_soft_argmin_fwd) has its own kernel: label the launch
        # with what the host code picks
        kname = lambda: soft_argmin_kernel_label(soft_argmin_fwd_plan_name(
            c4, disp, stats, B, Dc, Hc, Wc, D, H, W, negate, align_corners))
        with torch.cuda.device(cost.device), _timed(kname, 4.0 * B * (Dc * Hc * Wc + H * W)):
            rc = lib.dsm_soft_argmin_fwd(_p(c4), _p(disp), _p(stats), B, Dc, Hc, Wc, D, H, W,
                                         int(negate), int(align_corners), _lib.DSM_F32, _stream())
        _lib.check(rc, "dsm_soft_argmin_fwd")
        if need_grad:
            ctx.save_for_backward(c4, disp, stats)
        ctx.cfg = (tuple(cost.shape), B, Dc, Hc, Wc, D, H, W, int(negate), int(align_corners))
        return disp

    @staticmethod
    def backward(ctx, gdisp):
        c4, disp, stats = ctx.saved_tensors
        shape, B, Dc, Hc, Wc, D, H, W, negate, align = ctx.cfg
        g = gdisp.contiguous()
        dcost = torch.empty_like(c4)
        lib = _lib.load()
        with torch.cuda.device(c4.device):
            rc = lib.dsm_soft_argmin_bwd(_p(c4), _p(disp), _p(stats), _p(g), _p(dcost), B, Dc, Hc,
                                         Wc, D, H, W, negate, align, _lib.DSM_F32, _stream())
        _lib.check(rc, "dsm_soft_argmin_bwd")
        return dcost.reshape(shape), None, None, None


def soft_argmin_kernel_label(plan):
    """Timer label of a soft-argmin forward launch from its plan name."""
    return "soft_argmin_up4_kernel" if plan.startswith("up4") else "soft_argmin_fwd_kernel"


def soft_argmin(cost, out_size=None, negate=False, align_corners=False):
    """Fused (trilinear upsample ->) softmax over disparity -> expectation.  -> (B, H, W)."""
    return SoftArgminFunction.apply(cost, out_size, bool(negate), bool(align_corners))


DispConfidence = collections.namedtuple("DispConfidence", ("disp", "peak", "pmax", "pwin", "entropy"))


def soft_argmin_confidence(cost, out_size=None, negate=False, align_corners=False, radius=4,
                           want=("peak", "pmax", "pwin", "entropy")):
    """``soft_argmin`` plus what the softmax it regresses from says about each pixel, in one launch
    (csrc/soft_argmin.hip, ``dsm_disp_confidence_fwd``).  With ``p`` the softmax over the (upsampled)
    disparity axis and ``d*`` its first arg-max, all (B, H, W):

      disp     ``sum d p_d``, what ``soft_argmin`` returns
      peak     the same regression restricted to the window ``[d* - radius, d* + radius]`` (clipped to
               the range): it does not average across the modes of a bimodal distribution
      pmax     ``p_{d*}``
      pwin     the probability mass of that window
      entropy  ``-sum p_d ln p_d`` in nats, in ``[0, ln D]``

    ``cost``: (B,1,D,H,W) or (B,D,H,W) float32 on the device, as for ``soft_argmin``.  ``want``: the
    maps to compute besides ``disp``; the others are None.  Inference only: the outputs carry no graph,
    and a cost that requires grad (with gradients enabled) is refused.  Capturable: torch allocates,
    nothing synchronises."""
    _require_device("soft_argmin_confidence", cost)
    if cost.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("soft_argmin_confidence: inference only, there is no backward for these maps; "
                           "call it under torch.no_grad() or detach the cost")
    names = tuple(want)
    if any(n not in DispConfidence._fields[1:] for n in names):
        raise ValueError("soft_argmin_confidence: want is a subset of %s, got %r" % (DispConfidence._fields[1:], want))
    radius = int(radius)
    if radius < 0:
        raise ValueError("soft_argmin_confidence: radius must be >= 0, got %d" % radius)
    if cost.dim() == 5:
        if cost.shape[1] != 1:
            raise ValueError("soft_argmin_confidence: 5-D cost must have one channel")
        c4 = cost.reshape(cost.shape[0], *cost.shape[2:])
    elif cost.dim() == 4:
        c4 = cost
    else:
        raise ValueError("soft_argmin_confidence: expected (B,1,D,H,W) or (B,D,H,W)")
    c4 = c4.detach().contiguous()
    B, Dc, Hc, Wc = c4.shape
    D, H, W = (Dc, Hc, Wc) if out_size is None else tuple(int(v) for v in out_size)
    out = {n: torch.empty((B, H, W), device=cost.device, dtype=cost.dtype) for n in ("disp",) + names}
    lib = _lib.load()
    kname = lambda: ("disp_confidence_up4_kernel" if confidence_plan_name(
        c4, out["disp"], B, Dc, Hc, Wc, D, H, W, negate, align_corners, radius).startswith("conf_up4")
        else "disp_confidence_kernel")
    with torch.cuda.device(cost.device), _timed(kname, 4.0 * B * (Dc * Hc * Wc + len(out) * H * W)):
        rc = lib.dsm_disp_confidence_fwd(_p(c4), _p(out["disp"]), _p(out.get("peak")), _p(out.get("pmax")),
                                         _p(out.get("pwin")), _p(out.get("entropy")), B, Dc, Hc, Wc, D, H, W,
                                         int(bool(negate)), int(bool(align_corners)), min(radius, 2 ** 31 - 1),
                                         _lib.DSM_F32, _stream())
    _lib.check(rc, "dsm_disp_confidence_fwd")
    return DispConfidence(*[out.get(n) for n in DispConfidence._fields])


# ----------------------------------------------------------------------------
# (a4, a5) 3-D convolution block
# ----------------------------------------------------------------------------
def pack_conv3d_weight(weight, transposed):
    """torch Conv3d / ConvTranspose3d weight (k=3) -> MFMA fragment order (device)."""
    _require_device("pack_conv3d_weight", weight)
    if weight.dim() != 5 or tuple(weight.shape[2:]) != (3, 3, 3):
        raise ValueError("conv3d_block supports kernel_size=3 only, got %s" % (tuple(weight.shape),))
    cin, cout = (weight.shape[0], weight.shape[1]) if transposed else (weight.shape[1], weight.shape[0])
    w = weight.detach().contiguous()
    lib = _lib.load()
    nbytes = lib.dsm_conv3d_packed_weight_bytes(cin, cout, int(transposed))
    packed = torch.empty(nbytes // 4, device=w.device, dtype=torch.float32)
    with torch.cuda.device(w.device):
        rc = lib.dsm_conv3d_pack_weights(_p(w), _p(packed), cin, cout, int(transposed), _stream())
    _lib.check(rc, "dsm_conv3d_pack_weights")
    return packed


def to_channels_last_3d(x):
    """(B,C,D,H,W) in any strides -> NDHWC memory (no copy when it already is)."""
    if x.is_contiguous(memory_format=_CL3D):
        return x
    _require_device("to_channels_last_3d", x)
    xc = x.contiguous()
    B, C, D, H, W = xc.shape
    out = torch.empty((B, C, D, H, W), device=x.device, dtype=x.dtype, memory_format=_CL3D)
    with torch.cuda.device(x.device):
        rc = _lib.load().dsm_volume_relayout(_p(xc), _p(out), B, C, D, H, W, 1, _stream())
    _lib.check(rc, "dsm_volume_relayout")
    return out


def to_contiguous_3d(x):
    """NDHWC memory -> torch contiguous (B,C,D,H,W)."""
    if x.is_contiguous():
        return x
    if not x.is_contiguous(memory_format=_CL3D):
        return x.contiguous()
    B, C, D, H, W = x.shape
    out = torch.empty((B, C, D, H, W), device=x.device, dtype=x.dtype)
    with torch.cuda.device(x.device):
        rc = _lib.load().dsm_volume_relayout(_p(x), _p(out), B, C, D, H, W, 0, _stream())
    _lib.check(rc, "dsm_volume_relayout")
    return out


def conv3d_out_size(in_size, stride, transposed):
    if transposed:
        return tuple(2 * v for v in in_size)          # k3, s2, p1, op1
    return tuple((v - 1) // stride + 1 for v in in_size)


def conv3d_block(x, packed_weight, cout, scale=None, shift=None, residual=None, stride=1,
                 transposed=False, relu=False, out_size=None):
    """y = relu?(conv(x) * scale + shift (+ residual, cropped to the common size)).

    ``x`` is (B,Cin,D,H,W); it is consumed in NDHWC memory (converted if needed) and
    the result is returned as a channels_last_3d tensor.  With ``residual`` the output
    takes the element-wise minimum of the two spatial sizes -- ``myadd_3d`` semantics
    (stackhourglass.py:10-20).  ``x`` may be a ``VirtualVolume`` (Conv3d k3 s1 to 32 channels: the
    z-sliding kernel stages the never-materialised cost volume from the towers' output).
    Inference only.  What the MFMA kernels multiply in follows the ``conv_precision`` option."""
    virtual = x if isinstance(x, VirtualVolume) else None
    if virtual is not None:
        x = virtual.features                     # NHWC (2B, C, H, W): staged as the volume's planes
        if stride != 1 or transposed or cout != 32:
            raise ValueError("a virtual cost volume feeds a Conv3d(k3, s1) to 32 channels only")
        _require_device("conv3d_block", x, scale, shift, residual)
        B, cin, Di, Hi, Wi = virtual.shape
    else:
        _require_device("conv3d_block", x, scale, shift, residual)
        x = carry_amax(to_channels_last_3d(x), x)
        B, cin, Di, Hi, Wi = x.shape
    Do, Ho, Wo = conv3d_out_size((Di, Hi, Wi), stride, transposed)
    res_size = None
    if residual is not None:
        if residual.shape[0] != B or residual.shape[1] != cout:
            raise ValueError("conv3d_block: residual has shape %s, expected (%d,%d,...)"
                             % (tuple(residual.shape), B, cout))
        residual = to_channels_last_3d(residual)
        res_size = tuple(residual.shape[2:])
        Do, Ho, Wo = (min(n, r) for n, r in zip((Do, Ho, Wo), res_size))
    if out_size is not None:                     # a corner of the natural output (bwd-data crops)
        Do, Ho, Wo = (min(n, int(o)) for n, o in zip((Do, Ho, Wo), out_size))
    y = torch.empty((B, cout, Do, Ho, Wo), device=x.device, dtype=torch.float32, memory_format=_CL3D)
    # FLOPs as SURVEY.md section 8d counts them: 2*27*Cin*Cout per output voxel (conv) or
    # per input voxel (transposed conv)
    # (Cout = 1 runs on the VALU and is HBM-bound: input read once + output written)
    vox = B * (Di * Hi * Wi if transposed else Do * Ho * Wo)
    work = 54.0 * cin * cout * vox if cout > 1 else 4.0 * B * (cin * Di * Hi * Wi + Do * Ho * Wo)
    _conv_launch(x, packed_weight, scale, shift, residual, y, B, cin, cout, (Di, Hi, Wi), (Do, Ho, Wo), res_size,
                 stride, transposed, relu, work, virtual=virtual)
    return y


def conv3d_plan_name(args):
    """Kernel variant ``dsm_conv3d_fwd`` picks for ``args`` (``dsm_conv3d_plan``)."""
    return _plan_name("dsm_conv3d_plan", args)


def _conv_plan(args):
    """(rc, name) of ``dsm_conv3d_plan`` for a COPY of ``args`` in which every null one of ``x``, ``w_packed``, ``y``,
    ``x_amax`` is a stand-in aligned address (only NULL-ness and alignment are looked at): needs no tensors."""
    a = _lib.Conv3dArgs.from_buffer_copy(args)
    for field in ("x", "w_packed", "y", "x_amax"):
        if not getattr(a, field):
            setattr(a, field, 16)
    buf = ctypes.create_string_buffer(96)
    rc = _lib.load().dsm_conv3d_plan(ctypes.byref(a), buf, 96)
    return rc, buf.value.decode()


# ----------------------------------------------------------------------------
# host-side options, absolute maxima of the fp16 precisions, the virtual cost volume
# ----------------------------------------------------------------------------
# host-side options (the library itself reads no environment variable): "conv_precision" starts from
# DSM_CONV_PRECISION=bf16x3|fp32|f16x2|f16 so that scripts and the parity tests can switch whole runs
_PRECISIONS = ("bf16x3", "fp32", "f16x2", "f16")


def _env_precision():
    v = os.environ.get("DSM_CONV_PRECISION", "")
    if v and v not in _PRECISIONS:
        raise ValueError("DSM_CONV_PRECISION must be one of %s, got %r" % (_PRECISIONS, v))
    return v or "f16x2"


def _env_flag(name, default):
    v = os.environ.get(name, "")
    if v not in ("", "0", "1"):
        raise ValueError("%s must be 0 or 1, got %r" % (name, v))
    return default if v == "" else v == "1"


# ``wide_conv2d``: default from profiles/wide2d.md, whole DispNetC forward, option off
# against on in one process
_WIDE_CONV2D_DEFAULT = False

_OPTIONS = {"fuse_volume": True, "fuse_blocks": True, "conv_precision": _env_precision(), "conv_flags": 0,
            "separable_volume": _env_flag("DSM_SEPARABLE_VOLUME", True), "separable_flags": 0,
            "fused_supervised_loss": _env_flag("DSM_FUSED_SUP_LOSS", True),
            "wide_conv2d": _env_flag("DSM_WIDE_CONV2D", _WIDE_CONV2D_DEFAULT),
            "wide_conv2d_train": _env_flag("DSM_WIDE_CONV2D_TRAIN", False),
            "conv2d_k5": _env_flag("DSM_CONV2D_K5", False),
            "warp_train": _env_flag("DSM_WARP_TRAIN", False),
            "decoder_train": _env_flag("DSM_DECODER_TRAIN", False),
            "corr1d_tiled_bwd": False}


def set_option(name, value):
    """Host-side switches for A/B runs and tests (no environment variable is read by the library):
    ``conv_precision`` -- what the 3x3(x3) MFMA convolutions multiply in:
        "bf16x3"  fp32 accuracy, three-term bf16 split, six MFMAs per product;
        "f16x2"   fp32 accuracy, two-term fp16 split of power-of-two-scaled operands, three MFMAs;
        "f16"     operands rounded to fp16, one MFMA, fp32 accumulate -- the reduced-precision mode of
                  BASELINE config #5 (forward, backward-data and weight gradients);
        "fp32"    the exact fp32-input MFMA (v_mfma_f32_32x32x2_f32);
    ``conv_fp32`` -- older spelling: True = "fp32", False = "bf16x3";
    ``fuse_volume`` -- PSMNet's / GCNet's eval forward never materialises the cost volume: the first
    3-D convolution stages it from the feature maps;
    ``separable_volume`` -- the first 3-D convolution of a never-materialised volume runs as 2-D maps
    plus a broadcast (``concat_conv_block``) instead of the z-sliding kernel; starts from
    DSM_SEPARABLE_VOLUME=0|1 (default on); ``separable_flags``: raw tuning bits of dsm_concat_conv_fwd;
    ``fuse_blocks`` -- the towers' stride-1 64-channel BasicBlocks run as one launch each (fp16 modes);
    ``fused_supervised_loss`` -- ``train.losses("supervised")`` runs as ``supervised_pyramid_loss`` (three
    launches, csrc/suploss.hip) instead of stock torch ops; starts from DSM_FUSED_SUP_LOSS=0|1 (default on);
    ``wide_conv2d`` -- the 256 / 512 / 1024-channel 3x3 layers of the DispNetC / iResNet encoders run on the
    wide MFMA kernel (csrc/conv_wide2d.hpp; eval, fp16 modes) instead of the stock layer; starts from
    DSM_WIDE_CONV2D=0|1;
    ``wide_conv2d_train`` -- the same layers with Cin and Cout both in 256 / 512 / 1024 train on
    ``wide_conv2d_relu`` under autograd (forward, ReLU + bias backward, backward-data and weight gradient on
    this project's kernels; fp16 modes), whatever ``wide_conv2d`` says; default off (profiles/wide2d_train.md),
    starts from DSM_WIDE_CONV2D_TRAIN=0|1;
    ``conv2d_k5`` -- the 5x5 stride-2 layers to 128 / 256 channels with Cin % 16 == 0 (DispNet's conv2 and
    conv3a, the conv2 of DispNetC / iResNet) run on the MFMA kernel (csrc/conv_wide2d.hpp with a 5x5 window;
    eval, fp16 modes) instead of the stock layer; default off (profiles/conv2d_k5.md), starts from
    DSM_CONV2D_K5=0|1;
    ``warp_train`` -- iResNet's reconstruction error ``|stemL - imwrap_BCHW(stemR, -r_pr0)|`` runs as
    ``warp_abs_error`` under autograd too (fp32 GPU tensors; csrc/warp.hip forward and backward) instead of the
    stock grid_sample chain; default off (profiles/train_ops.md), starts from DSM_WARP_TRAIN=0|1;
    ``decoder_train`` -- ``decoder_level`` keeps its one-launch bias + ReLU + upsampling + concatenation under
    autograd (``DecoderCatFunction``, csrc/decoder.hip forward and backward); independent of ``warp_train``;
    default off (profiles/train_ops.md), starts from DSM_DECODER_TRAIN=0|1;
    ``corr1d_tiled_bwd`` -- the backward of the dot-product ``corr1d`` goes through ``dsm_corr1d_sim_bwd`` (the
    LDS-tiled data gradient where its plan admits it) instead of ``dsm_corr1d_bwd``; default off
    (profiles/corr1d_sim.md).  The cosine similarity always takes that entry point;
    ``conv_flags`` -- raw dsm_conv3d_args.flags bits (tile height, grid size, K-ranges of the wide layers)."""
    if name == "conv_fp32":
        old = _OPTIONS["conv_precision"] == "fp32"
        _OPTIONS["conv_precision"] = "fp32" if value else "bf16x3"
        return old
    if name not in _OPTIONS:
        raise KeyError(name)
    old = _OPTIONS[name]
    if name == "conv_precision":
        if value not in _PRECISIONS:
            raise ValueError("conv_precision must be one of %s" % (_PRECISIONS,))
        _OPTIONS[name] = value
    else:
        _OPTIONS[name] = int(value) if name in ("conv_flags", "separable_flags") else bool(value)
    return old


def _mode(mode):
    """The precision mode a launch runs in: ``mode``, or (None) the ``conv_precision`` option.  A backward that
    must match its forward passes the forward's; nothing swaps the option, which every thread reads."""
    return _OPTIONS["conv_precision"] if mode is None else mode


def _conv_flags(mode=None):
    """dsm_conv3d_args.flags of every convolution launch: precision "fp32" keeps the exact fp32-input
    MFMA kernels; ``conv_flags`` carries raw A/B bits (tile height, grid size: include/dsmnet_hip.h)."""
    return (_lib.DSM_CONV_FP32_MFMA if _mode(mode) == "fp32" else 0) | _OPTIONS["conv_flags"]


def get_option(name):
    if name == "conv_fp32":
        return _OPTIONS["conv_precision"] == "fp32"
    return _OPTIONS[name]


# ----------------------------------------------------------------------------
# absolute maxima for the fp16 precisions (include/dsmnet_hip.h: x_amax / y_amax)
# ----------------------------------------------------------------------------
# The fp16 split kernels scale every tensor by a power of two taken from its absolute maximum -- a
# device float that the PRODUCING launch writes from its epilogue (atomic max) and the consumer
# reads at kernel start: no host round trip, capturable in a hipGraph.  On the host the scalar rides
# on the tensor object as ``_dsm_amax``; a tensor without one (an input of the model, the result of
# a stock torch op) gets it from one ``dsm_absmax`` pass.  Slots come from a per-device arena that a
# model forward zeroes once (``amax_scope``), so that a forward costs one fill, not one per layer.
#
# A slot outlives the launch that wrote it only as long as its arena is not begun again: every
# ``begin`` zeroes the buffer and hands the same addresses out anew, while tensors of the earlier
# scope (an input saved for backward, an output the caller kept) still carry their slot.  Each slot
# therefore remembers the generation of the arena it was cut from, and ``amax_of`` serves it only
# while that is still the arena's generation; a stale one is replaced by a fresh ``dsm_absmax`` pass
# over the tensor.  All of it is host book-keeping: no device value is read, a captured ``begin``
# stays one memset inside the graph, and a slot that is valid costs nothing extra.  (DESIGN.md
# section 9, "state that outlives a launch")
class _AmaxArena(object):
    """``depth``, ``used`` and ``generation`` are per device: a scope opened for one device neither
    continues nor skips the ``begin`` of another's.  Process-wide on purpose, not thread-local: the
    backward of a step runs on autograd's device thread and must see the scope its forward opened."""
    SLOTS = 2048

    def __init__(self):
        self.buf, self.used, self.depth, self.generation = {}, {}, {}, {}

    @staticmethod
    def key(device):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:          # "cuda" is the current device
            return (device.type, torch.cuda.current_device())
        return (device.type, device.index)

    def begin(self, device):
        key = self.key(device)
        if key not in self.buf:
            self.buf[key] = torch.zeros(self.SLOTS, device=device, dtype=torch.float32)
        else:
            self.buf[key].zero_()
        self.used[key] = 0
        self.generation[key] = self.generation.get(key, 0) + 1      # every slot handed out before is stale

    def enter(self, device):
        key = self.key(device)
        if self.depth.get(key, 0) == 0:
            self.begin(device)
        self.depth[key] = self.depth.get(key, 0) + 1

    def leave(self, device):
        self.depth[self.key(device)] -= 1

    def slot(self, device):
        """A zeroed float for one launch to write a maximum into: the next slot of the open scope's
        arena, or -- outside any scope, or past ``SLOTS`` -- a private scalar that nothing invalidates."""
        key = self.key(device)
        if self.depth.get(key, 0) > 0 and self.used[key] < self.SLOTS:
            i = self.used[key]
            self.used[key] = i + 1
            s = self.buf[key][i:i + 1]
            s._dsm_generation = (key, self.generation[key])
            return s
        return torch.zeros(1, device=device, dtype=torch.float32)

    def valid(self, slot):
        """Does ``slot`` still hold what its producer wrote (its arena has not been begun again)?"""
        tag = getattr(slot, "_dsm_generation", None)
        return tag is None or self.generation.get(tag[0]) == tag[1]


_ARENA = _AmaxArena()


class amax_scope(object):
    """``with amax_scope(device):`` around a model forward: the absolute-maximum slots of every
    launch inside come from one arena, zeroed once on entry (nested scopes share the outer one, and
    leaving the inner one changes nothing).  Entering an outermost scope ends the validity of every
    slot the device's arena handed out before: ``amax_of`` recomputes those.  A no-op unless an fp16
    precision is selected."""

    def __init__(self, device):
        self.device = device

    def __enter__(self):
        if needs_amax():
            _ARENA.enter(self.device)
            self.entered = True
        else:
            self.entered = False
        return self

    def __exit__(self, *exc):
        if self.entered:
            _ARENA.leave(self.device)
        return False


def needs_amax(mode=None):
    return _mode(mode) in ("f16x2", "f16")


def absmax(x):
    """Device scalar holding exactly ``x.abs().max()`` (``dsm_absmax``), also remembered on ``x``.

    ``dsm_absmax`` scans ``numel()`` floats from a 16-byte-aligned address, so:
      * a dtype other than float32 raises ``TypeError`` before any launch;
      * a tensor that does not own a dense block of memory (a channel or spatial slice, an expanded
        tensor) is reduced over ``x.contiguous()``: one copy, the exact maximum of the elements of
        ``x`` and of nothing else;
      * a dense view at a storage offset that is not 16-byte aligned is reduced over a copy too.
    A dense tensor in any dimension order (channels_last included) is scanned in place.  An empty
    tensor raises ``ValueError``.  ``amax_of`` inherits all of this."""
    if x.dtype != torch.float32:
        raise TypeError("absmax: float32 only, got %s" % (x.dtype,))
    if x.numel() == 0:
        raise ValueError("absmax of an empty tensor")
    src = x.detach()
    if not _dense(src):
        src = src.contiguous()
    if src.data_ptr() % 16:
        src = src.clone(memory_format=torch.contiguous_format)
    slot = _ARENA.slot(x.device)
    with torch.cuda.device(x.device), _timed("absmax_kernel", 4.0 * x.numel()):
        rc = _lib.load().dsm_absmax(_p(src), src.numel(), _p(slot), _stream())
    _lib.check(rc, "dsm_absmax")
    try:
        x._dsm_amax = slot
    except AttributeError:
        pass
    return slot


def _dense(x):
    """Do the elements of ``x`` fill one block of ``numel()`` elements, each address once (any order)?"""
    if x.is_contiguous():
        return True
    expect = 1
    for size, stride in sorted(((n, s) for n, s in zip(x.shape, x.stride()) if n != 1), key=lambda t: t[1]):
        if stride != expect:
            return False
        expect *= size
    return True


def amax_of(x):
    """The absolute-maximum scalar of ``x``: the one its producer attached, while the arena it was cut
    from has not been begun again (``amax_scope``); else a fresh pass (``absmax``)."""
    slot = getattr(x, "_dsm_amax", None)
    return slot if slot is not None and _ARENA.valid(slot) else absmax(x)


def carry_amax(dst, *srcs):
    """``dst`` holds values bounded by the maximum over ``srcs`` (a view, a slice, a concatenation):
    hand the bound on without a pass when a single source carries one.  The slot object itself is
    handed on, and its validity with it: the bound of ``dst`` goes stale when its source's does."""
    slots = [getattr(t, "_dsm_amax", None) for t in srcs]
    if len(slots) == 1 and slots[0] is not None:
        dst._dsm_amax = slots[0]
    return dst


WIDE2D_COUT = (256, 512, 1024)
K5_COUT = (128, 256)            # the 5x5 stride-2 layers (plan kind 10)


def _split_kernel_layer(a):
    """Does ``dsm_conv3d_fwd`` run ``a`` (precision and flags set) on a kernel that reads ``x_amax``?  The planner's
    own answer: such a plan carries its mode in its name (include/dsmnet_hip.h).  False for a refused plan."""
    rc, name = _conv_plan(a)
    return rc == _lib.DSM_OK and ("_f16x2_" in name or "_f16_" in name)


def _set_precision(a, x, y, mode=None):
    """precision / x_amax / y_amax of a ``dsm_conv3d_args``.  Returns the tensors the launch must
    keep alive.  ``x``, ``y``: the input and output tensors (NDHWC / NHWC memory); ``y`` None:
    the output needs no maximum (Cout = 1 heads)."""
    mode = _mode(mode)
    if mode not in ("f16x2", "f16"):
        return None
    a.precision = _lib.DSM_PREC_F16X2 if mode == "f16x2" else _lib.DSM_PREC_F16
    xa = None
    if _split_kernel_layer(a):                       # the others compute in fp32 and read no maximum
        xa = amax_of(x)
        a.x_amax = xa.data_ptr()
    ya = None
    if y is not None:
        ya = _ARENA.slot(y.device)
        a.y_amax = ya.data_ptr()
        y._dsm_amax = ya
    return xa, ya


def _conv_launch(x, packed_weight, scale, shift, residual, y, B, cin, cout, in_size, out_size, res_size, stride,
                 transposed, relu, work, kd=0, k=0, dil=0, virtual=None, mode=None):
    """The ``dsm_conv3d_fwd`` call of ``conv3d_block``, ``conv2d_block`` and ``conv2d_transposed_block``, which
    have converted the layouts, worked out the extents and allocated ``y``.  ``in_size`` / ``out_size`` /
    ``res_size``: (D, H, W) of ``x`` / ``y`` / ``residual`` (None without one); ``kd``, ``k``, ``dil``: 0 is the
    struct's default (3 x 3 x 3 taps, dilation 1); ``virtual``: the ``VirtualVolume`` that ``x`` holds the
    features of; ``work``: the launch's FLOPs or bytes for the timer; ``mode``: see ``_mode``."""
    a = _lib.Conv3dArgs()
    a.x, a.w_packed, a.y = _p(x), _p(packed_weight), _p(y)
    a.scale, a.shift, a.residual = _p(scale), _p(shift), _p(residual)
    a.B, a.Cin, a.Cout = B, cin, cout
    a.Di, a.Hi, a.Wi = in_size
    a.Do, a.Ho, a.Wo = out_size
    if res_size is not None:
        a.Dr, a.Hr, a.Wr = res_size
    a.stride, a.transposed, a.relu = int(stride), int(transposed), int(relu)
    a.kd, a.k, a.dil = int(kd), int(k), int(dil)
    a.flags = _conv_flags(mode)
    if virtual is not None:
        a.vol_virtual, a.vol_mask_left = 1, int(virtual.mask_left)
    keep = _set_precision(a, x, y if cout > 1 else None, mode)
    lib = _lib.load()
    ws = None
    if kd == 1 and (cout in WIDE2D_COUT or k == 5):
        # the wide (and 5x5) layers' K-split partial sums: from torch's caching allocator, per call (no
        # synchronisation; inside a hipGraph capture the block belongs to the graph's pool).  Asked for
        # these layers only: the query runs the planner
        nws = lib.dsm_conv3d_workspace_bytes(ctypes.byref(a))
        if nws:
            ws = torch.empty(nws // 4, device=y.device, dtype=torch.float32)
            a.workspace, a.workspace_bytes = ws.data_ptr(), nws
    with torch.cuda.device(y.device), _timed(lambda: _plan_name("dsm_conv3d_plan", a), work):
        rc = lib.dsm_conv3d_fwd(ctypes.byref(a), _stream())
    _lib.check(rc, "dsm_conv3d_fwd")
    del keep, ws                                     # alive until the call has returned


class VirtualVolume(object):
    """A concatenation cost volume that is never written (models/psmnet/stackhourglass.py:124-133,
    models/gcnet.py:130-135): ``features`` is the towers' output for both views as ONE NHWC tensor
    (2B, C, H, W) [left maps, then right maps]; the first 3-D convolution (``conv3d_block``; the
    z-sliding kernel, csrc/conv_zs.hpp) stages plane d as [left | right shifted by d] with x < d
    zeroed.  ``shape``: the logical (B, 2C, D, H, W).  Inference only."""
    __slots__ = ("features", "shape", "mask_left")

    def __init__(self, features, D, mask_left):
        if features.dim() != 4 or features.shape[0] % 2:
            raise ValueError("VirtualVolume: features must be (2B, C, H, W), left maps then right maps")
        if not features.is_contiguous(memory_format=torch.channels_last):
            features = carry_amax(features.contiguous(memory_format=torch.channels_last), features)
        self.features = features
        B2, C, H, W = features.shape
        self.shape = (B2 // 2, 2 * C, int(D), H, W)
        self.mask_left = bool(mask_left)

    @property
    def device(self):
        return self.features.device


def virtual_volume_ok(C):
    """The z-sliding kernel can stage a virtual volume of 2C channels (C % 32 == 0) in every
    precision except "fp32" (which has no split kernels)."""
    return C % 32 == 0 and _OPTIONS["conv_precision"] != "fp32"


# ----------------------------------------------------------------------------
# first convolution of a virtual cost volume from 2-D maps (csrc/sepvol.hip)
# ----------------------------------------------------------------------------
def pack_concat_conv_weight(weight):
    """Conv3d weight (32, 2C, 3, 3, 3) of the layer that reads a concatenation volume ->
    [side][dz][dx][dy][C/2][2][32] (flat): the operand order of ``dsm_concat_conv_fwd``'s column
    convolutions -- input channel ``side*C + h*C/2 + cc`` sits at [..][cc][h][..].  A pure
    permutation (no sums), any device."""
    if weight.dim() != 5 or tuple(weight.shape[2:]) != (3, 3, 3) or weight.shape[1] % 4:
        raise ValueError("pack_concat_conv_weight: expected (Cout, 2C, 3, 3, 3) with C even, got %s"
                         % (tuple(weight.shape),))
    cout, c2 = weight.shape[:2]
    w = weight.detach().reshape(cout, 2, 2, c2 // 4, 3, 3, 3)         # o, side, h, cc, dz, dy, dx
    return w.permute(1, 4, 6, 5, 3, 2, 0).contiguous().reshape(-1)


def concat_conv_ok(x, cout, stride=1, transposed=False):
    """Does ``concat_conv_block`` cover this layer (else: ``conv3d_block`` on the z-sliding kernel)?"""
    return (_OPTIONS["separable_volume"] and isinstance(x, VirtualVolume) and cout == 32 and stride == 1 and
            not transposed and x.shape[1] // 2 in (32, 64) and x.shape[0] * x.shape[3] <= 65535)


def concat_conv_workspace_floats(B, H, W):
    return 32 * H * (18 * B * W + 4 * B * (2 * W + 2))


def concat_conv_block(x, sep_weight, scale=None, shift=None, relu=False):
    """y = relu?(conv3d(volume) * scale + shift) for a ``VirtualVolume`` ``x`` and a Conv3d(2C -> 32, k3,
    s1, p1) whose weight was packed by ``pack_concat_conv_weight``: the volume's planes are shifted
    copies of two 2-D maps, so the convolution is 2-D column convolutions of the towers' output
    (fp32-input MFMA), their sums F and G, and one pass that writes F[y, x] + G[y, x - d] (the general
    18-term form at the borders) -- three launches, no volume, no 3-D arithmetic.  Independent of
    ``conv_precision``; the result carries its exact absolute maximum in the fp16 modes.
    Returns (B, 32, D, H, W) channels_last_3d.  Inference only."""
    if not isinstance(x, VirtualVolume):
        raise TypeError("concat_conv_block takes a VirtualVolume")
    both = x.features
    _require_device("concat_conv_block", both, sep_weight, scale, shift)
    B, c2, D, H, W = x.shape
    C = c2 // 2
    if sep_weight.numel() != 27 * 32 * c2:
        raise ValueError("concat_conv_block: packed weight has %d floats, expected %d"
                         % (sep_weight.numel(), 27 * 32 * c2))
    y = torch.empty((B, 32, D, H, W), device=both.device, dtype=torch.float32, memory_format=_CL3D)
    nws = concat_conv_workspace_floats(B, H, W)
    ws = torch.empty(nws, device=both.device, dtype=torch.float32)
    ya = _ARENA.slot(both.device) if needs_amax() else None
    # HBM-side bytes: the features in, the output out (the K / F / G workspace stays in the caches)
    work = 4.0 * (both.numel() + y.numel())
    with torch.cuda.device(both.device), _timed("sepvol_fwd_kernel", work):
        rc = _lib.load().dsm_concat_conv_fwd(_p(both), _p(sep_weight), _p(scale), _p(shift), _p(ws), nws,
                                             _p(y), _p(ya), B, C, 32, D, H, W, int(x.mask_left),
                                             int(bool(relu)), _OPTIONS["separable_flags"], _stream())
    _lib.check(rc, "dsm_concat_conv_fwd")
    if ya is not None:
        y._dsm_amax = ya
    return y


# ----------------------------------------------------------------------------
# 2-D convolution block (feature towers): same MFMA kernel, kd = 1
# ----------------------------------------------------------------------------
_CL2D = torch.channels_last


def pack_conv2d_weight(weight, cin_padded=None):
    """torch Conv2d weight (Cout, Cin, k, k), k in {1, 3} -> MFMA fragment order.  ``cin_padded``
    (a multiple of 16 >= Cin) zero-fills the extra input channels.  k = 5 (Cout 128 / 256, Cin % 16 == 0): the
    fp16 section of the 5x5 stride-2 kernel alone."""
    _require_device("pack_conv2d_weight", weight)
    cout, cin, kh, kw = weight.shape
    if kh != kw or kh not in (1, 3, 5):
        raise ValueError("conv2d_block supports 1x1, 3x3 and 5x5 kernels, got %dx%d" % (kh, kw))
    cin_p = cin if cin_padded is None else int(cin_padded)
    w = weight.detach().contiguous()
    lib = _lib.load()
    nbytes = lib.dsm_conv_packed_weight_bytes(cin_p, cout, 1, kh)
    if nbytes == 0:
        raise ValueError("pack_conv2d_weight: unsupported shape %s" % (tuple(weight.shape),))
    packed = torch.empty(nbytes // 4, device=w.device, dtype=torch.float32)
    with torch.cuda.device(w.device):
        rc = lib.dsm_conv_pack_weights(_p(w), _p(packed), cin, cin_p, cout, 1, kh, _stream())
    _lib.check(rc, "dsm_conv_pack_weights")
    return packed


def conv2d_block(x, packed_weight, cout, scale=None, shift=None, residual=None, stride=1,
                 relu=0, k=3, dilation=1, mode=None):
    """y = relu?(conv2d(x) * scale + shift (+ residual)) on NHWC maps, "same" padding.
    ``x``: (B, Cin, H, W) in torch.channels_last memory, Cin a multiple of 16.  ``k`` = 5: stride 2 to 128 / 256
    channels in the fp16 modes, no residual.  Inference only."""
    _require_device("conv2d_block", x, packed_weight, scale, shift, residual)
    if not x.is_contiguous(memory_format=_CL2D):
        x = carry_amax(x.contiguous(memory_format=_CL2D), x)
    B, cin, Hi, Wi = x.shape
    Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
    if residual is not None:
        if tuple(residual.shape) != (B, cout, Ho, Wo):
            raise ValueError("conv2d_block: residual shape %s != %s"
                             % (tuple(residual.shape), (B, cout, Ho, Wo)))
        if not residual.is_contiguous(memory_format=_CL2D):
            residual = residual.contiguous(memory_format=_CL2D)
    y = torch.empty((B, cout, Ho, Wo), device=packed_weight.device, dtype=torch.float32, memory_format=_CL2D)
    _conv_launch(x, packed_weight, scale, shift, residual, y, B, cin, cout, (1, Hi, Wi), (1, Ho, Wo),
                 None if residual is None else (1, Ho, Wo), stride, False, relu,
                 2.0 * k * k * cin * cout * B * Ho * Wo, kd=1, k=k, dil=dilation, mode=mode)
    return y


def conv2d_k5_plan_ok(B, cin, cout, Hi, Wi, mode=None):
    """Does ``dsm_conv3d_plan`` admit Conv2d(cin -> cout, k5, pad 2, stride 2) on a (B, cin, Hi, Wi) map in precision
    ``mode``?  The host-only query: the geometry and offset limits are the library's, not a copy of them."""
    return _conv_plan(_conv2d_standin(B, cin, cout, Hi, Wi, 2, 5, 1, _mode(mode), _conv_flags(mode)))[0] == _lib.DSM_OK


def _conv2d_standin(B, cin, cout, Hi, Wi, stride, k, dil, mode, flags):
    """``dsm_conv3d_args`` of Conv2d(cin -> cout, k, "same" padding) on a (B, cin, Hi, Wi) map, for ``_conv_plan``."""
    a = _lib.Conv3dArgs()
    a.B, a.Cin, a.Cout = int(B), int(cin), int(cout)
    a.Di, a.Hi, a.Wi = 1, int(Hi), int(Wi)
    a.Do, a.Ho, a.Wo = 1, (int(Hi) - 1) // stride + 1, (int(Wi) - 1) // stride + 1
    a.stride, a.relu, a.kd, a.k, a.dil = int(stride), 1, 1, int(k), int(dil)
    a.precision = {"f16x2": _lib.DSM_PREC_F16X2, "f16": _lib.DSM_PREC_F16}.get(mode, _lib.DSM_PREC_F32)
    a.flags = flags
    return a


def conv2d_transposed_block(x, packed_weight, cout, out_size, mode=None):
    """Backward-data of a stride-2 wide layer (plan kind 9 of ``dsm_conv3d_fwd``, the transposed mode of the
    wide kernel): ``conv_transpose2d(x, W, stride 2, padding 1, output_padding 1)[:, :, :Ho, :Wo]`` with
    ``packed_weight`` the pack of the flipped, in/out-transposed ``W`` and ``out_size`` = (Ho, Wo), the extent
    of the tensor whose gradient this is (2 Hi - 1 <= Ho <= 2 Hi).  ``x``: (B, Cin, Hi, Wi) channels_last,
    Cin % 16 == 0; ``cout`` in 256 / 512 / 1024; fp16 precision modes only."""
    _require_device("conv2d_transposed_block", x, packed_weight)
    if not x.is_contiguous(memory_format=_CL2D):
        x = carry_amax(x.contiguous(memory_format=_CL2D), x)
    B, cin, Hi, Wi = x.shape
    Ho, Wo = int(out_size[0]), int(out_size[1])
    if not (2 * Hi - 1 <= Ho <= 2 * Hi and 2 * Wi - 1 <= Wo <= 2 * Wi):
        raise ValueError("conv2d_transposed_block: output %s is no stride-2 source of %s"
                         % ((Ho, Wo), (Hi, Wi)))
    y = torch.empty((B, cout, Ho, Wo), device=packed_weight.device, dtype=torch.float32, memory_format=_CL2D)
    _conv_launch(x, packed_weight, None, None, None, y, B, cin, cout, (1, Hi, Wi), (1, Ho, Wo), None, 2, True, 0,
                 18.0 * cin * cout * B * Ho * Wo, kd=1, k=3, dil=1, mode=mode)
    return y


def bias_relu_bwd(gy, y, need_db=True, mode=None):
    """``g = where(y > 0, gy, 0)`` as a tensor of its own (``gy`` is never written), ``db = g.sum over pixels``
    in a fixed order (or None) and, in the fp16 modes, the maximum of ``|g|`` attached to ``g`` -- one pass,
    ``dsm_bias_relu_bwd`` (csrc/relu_bwd.hip).  ``gy``, ``y``: (B, C, H, W) channels_last, C % 4 == 0."""
    _require_device("bias_relu_bwd", gy, y)
    _same_shape("bias_relu_bwd", gy, y)
    if not gy.is_contiguous(memory_format=_CL2D):
        gy = gy.contiguous(memory_format=_CL2D)
    if not y.is_contiguous(memory_format=_CL2D):
        y = y.contiguous(memory_format=_CL2D)
    B, C, H, W = y.shape
    M = B * H * W
    g = torch.empty((B, C, H, W), device=y.device, dtype=torch.float32, memory_format=_CL2D)
    db = ws = ga = None
    if need_db:
        db = torch.empty(C, device=y.device, dtype=torch.float32)
        ws = torch.empty(min(512, (M + 7) // 8) * C, device=y.device, dtype=torch.float32)
    if needs_amax(mode):
        ga = _ARENA.slot(y.device)
        g._dsm_amax = ga
    with torch.cuda.device(y.device), _timed("dsm_bias_relu_bwd", 0.0):
        rc = _lib.load().dsm_bias_relu_bwd(_p(gy), _p(y), _p(g), _p(db), _p(ws), _p(ga), M, C, _stream())
    _lib.check(rc, "dsm_bias_relu_bwd")
    return g, db


def basicblock2d_ok(x, cin, cout, stride, dilation):
    """Can a BasicBlock (two 3x3 convolutions + skip add) run as ONE launch (csrc/basicblock2d.hpp)?
    The towers' stride-1 64-channel blocks in the fp16 modes, eval."""
    return (_OPTIONS["fuse_blocks"] and _OPTIONS["conv_precision"] in ("f16x2", "f16") and cin in (32, 64) and
            cout == cin and stride == 1 and dilation == 1 and x.dim() == 4 and x.shape[1] == cin and
            4 * x.numel() < 2 ** 31)


def basicblock2d(x, packed1, scale1, shift1, packed2, scale2, shift2, relu=False, skip=True):
    """``conv2(relu(conv1(x) * scale1 + shift1)) * scale2 + shift2 + x`` (``relu``: ReLU after the add)
    on an NHWC map with 64 or 32 channels, both convolutions 3x3 / stride 1 / pad 1
    (models/psmnet/submodule.py:24-46, models/util_conv.py:181-210 with the BatchNorms folded;
    ``skip=False``: no ``+ x`` -- two convbn + ReLU layers in a row): one
    launch, the intermediate map stays in LDS.  ``packed*``: the layers' ``pack_conv2d_weight``
    buffers.  Inference only; fp16 modes only."""
    _require_device("basicblock2d", x, packed1, packed2, scale1, shift1, scale2, shift2)
    if not x.is_contiguous(memory_format=_CL2D):
        x = carry_amax(x.contiguous(memory_format=_CL2D), x)
    B, C, H, W = x.shape
    mode = _OPTIONS["conv_precision"]
    if C not in (32, 64) or mode not in ("f16x2", "f16"):
        raise ValueError("basicblock2d: 32 or 64 channels and an fp16 precision mode, got C=%d, %s" % (C, mode))
    y = torch.empty((B, C, H, W), device=x.device, dtype=torch.float32, memory_format=_CL2D)
    a = _lib.BasicBlock2dArgs()
    a.x, a.y = _p(x), _p(y)
    a.w1_packed, a.w2_packed = _p(packed1), _p(packed2)
    a.scale1, a.shift1, a.scale2, a.shift2 = _p(scale1), _p(shift1), _p(scale2), _p(shift2)
    a.B, a.H, a.W, a.C = B, H, W, C
    a.relu = 1 if relu else 0
    a.no_skip = 0 if skip else 1
    a.precision = _lib.DSM_PREC_F16X2 if mode == "f16x2" else _lib.DSM_PREC_F16
    xa = amax_of(x)
    ya = _ARENA.slot(y.device)
    a.x_amax, a.y_amax = xa.data_ptr(), ya.data_ptr()
    y._dsm_amax = ya
    work = 2.0 * 2 * 9 * C * C * B * H * W
    with torch.cuda.device(x.device), _timed("basicblock2d_%s_mfma_kernel<C=%d>" % (mode, C), work):
        rc = _lib.load().dsm_basicblock2d_fwd(ctypes.byref(a), _stream())
    _lib.check(rc, "dsm_basicblock2d_fwd")
    del xa
    return y


def warp_abs_error(left, right, disp, delt):
    """``|left - imwrap_BCHW(right, disp)|`` in one pass (csrc/warp.hip; utils/imwrap.py:37-72,
    models/iresnet.py:169-170).  ``left=None``: the warped map itself.  ``delt`` is the
    reference's random epsilon (a Python float drawn by the caller).  NCHW fp32.  With autograd on and
    an input that requires grad, the same launch runs inside ``WarpAbsErrorFunction``."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (left, right, disp)):
        return WarpAbsErrorFunction.apply(left, right, disp, float(delt))
    return _warp_abs_error_fwd(left, right, disp, delt)


def _warp_abs_error_fwd(left, right, disp, delt):
    _require_device("warp_abs_error", right, disp, left)
    B, C, H0, W0 = right.shape
    if disp.dim() != 4 or disp.shape[0] != B or disp.shape[1] != 1:
        raise ValueError("warp_abs_error: disp must be (B,1,H,W), got %s" % (tuple(disp.shape),))
    H, W = disp.shape[2:]
    if min(H, W, H0, W0) <= 1:
        raise ValueError("warp_abs_error: maps must be larger than 1x1")        # imwrap.py:48
    if left is not None and tuple(left.shape) != (B, C, H, W):
        raise ValueError("warp_abs_error: left %s does not match (B,C)=%s and disp %s"
                         % (tuple(left.shape), (B, C), (H, W)))
    right, disp = right.contiguous(), disp.contiguous()
    left = None if left is None else left.contiguous()
    out = torch.empty((B, C, H, W), device=right.device, dtype=torch.float32)
    n = out.numel()
    with torch.cuda.device(right.device), _timed("warp_abs_error_kernel",
                                                 4.0 * (right.numel() + disp.numel() + n * (2 if left is not None else 1))):
        rc = _lib.load().dsm_warp_abs_error(None if left is None else _p(left), _p(right), _p(disp),
                                            _p(out), B, C, H, W, H0, W0, float(delt), _stream())
    _lib.check(rc, "dsm_warp_abs_error")
    return out


class WarpAbsErrorFunction(torch.autograd.Function):
    """``warp_abs_error`` under autograd.  The forward is the eval launch (the same bits); the backward is
    one call of ``dsm_warp_abs_error_bwd``, which recomputes the warp from the saved inputs: ``gL`` and
    ``gdisp`` are written by one thread each, ``gR`` is an fp32 atomic scatter into a buffer the call zeroes."""

    @staticmethod
    def forward(ctx, left, right, disp, delt):
        out = _warp_abs_error_fwd(left, right, disp, delt)
        ctx.has_left, ctx.delt = left is not None, float(delt)
        ctx.save_for_backward(right.contiguous(), disp.contiguous(), *([left.contiguous()] if ctx.has_left else []))
        return out

    @staticmethod
    def backward(ctx, g):
        right, disp = ctx.saved_tensors[:2]
        left = ctx.saved_tensors[2] if ctx.has_left else None
        need_l, need_r, need_d = ctx.needs_input_grad[:3]
        B, C, H0, W0 = right.shape
        H, W = disp.shape[2:]
        g = g.contiguous()
        gl = torch.empty_like(left) if (need_l and ctx.has_left) else None
        gr = torch.empty_like(right) if need_r else None          # zeroed by the call
        gd = torch.empty_like(disp) if need_d else None
        work = 4.0 * (g.numel() * (1 + int(ctx.has_left) + int(gl is not None)) + right.numel() + disp.numel() +
                      (2 * right.numel() if need_r else 0) + (disp.numel() if need_d else 0))   # gR: zeroed, summed
        with torch.cuda.device(right.device), _timed("warp_abs_error_bwd_kernel", work):
            rc = _lib.load().dsm_warp_abs_error_bwd(_p(g), _p(left), _p(right), _p(disp), _p(gl), _p(gr), _p(gd),
                                                    B, C, H, W, H0, W0, ctx.delt, _stream())
        _lib.check(rc, "dsm_warp_abs_error_bwd")
        return gl, gr, gd, None


def spp_head(raw, skip, w_t, scale, shift):
    """PSMNet's SPP head in three launches (csrc/spp.hip; models/psmnet/submodule.py:81-99,
    126-137): ``raw`` (B,64,H,W) and ``skip`` (B,128,H,W) channels_last -> the 320-channel
    concat [raw | skip | branch4 | branch3 | branch2 | branch1] (B,320,H,W) channels_last.
    ``w_t`` (4,128,32): the branch4..branch1 1x1 weights, input-channel major; ``scale`` /
    ``shift`` (4,32): their folded BN.  Inference only."""
    _require_device("spp_head", raw, skip, w_t, scale, shift)
    B, cr, H, W = raw.shape
    if cr != 64 or tuple(skip.shape) != (B, 128, H, W):
        raise ValueError("spp_head: expected raw (B,64,H,W) and skip (B,128,H,W), got %s and %s"
                         % (tuple(raw.shape), tuple(skip.shape)))
    if tuple(w_t.shape) != (4, 128, 32) or tuple(scale.shape) != (4, 32) or tuple(shift.shape) != (4, 32):
        raise ValueError("spp_head: w_t (4,128,32), scale/shift (4,32) expected")
    if H < 64 or W < 64:
        raise ValueError("spp_head: the 64x64 pooling branch needs H, W >= 64 at 1/4 resolution "
                         "(got %dx%d)" % (H, W))
    raw = raw.contiguous(memory_format=_CL2D)
    skip = skip.contiguous(memory_format=_CL2D)
    w_t, scale, shift = w_t.contiguous(), scale.contiguous(), shift.contiguous()
    lib = _lib.load()
    h8, w8 = H // 8, W // 8
    p8 = torch.empty((B, h8, w8, 128), device=raw.device, dtype=torch.float32)
    br = torch.empty(lib.dsm_spp_branch_floats(B, h8, w8), device=raw.device, dtype=torch.float32)
    out = torch.empty((B, 320, H, W), device=raw.device, dtype=torch.float32, memory_format=_CL2D)
    with torch.cuda.device(raw.device):
        with _timed("spp_pool8_kernel", 4.0 * (skip.numel() + p8.numel())):
            rc = lib.dsm_spp_pool8(_p(skip), _p(p8), B, H, W, _stream())
        _lib.check(rc, "dsm_spp_pool8")
        with _timed("spp_branches_kernel", 4.0 * (p8.numel() + br.numel())):
            rc = lib.dsm_spp_branches(_p(p8), _p(w_t), _p(scale), _p(shift), _p(br), B, h8, w8,
                                      _stream())
        _lib.check(rc, "dsm_spp_branches")
        with _timed("spp_concat_kernel", 4.0 * (raw.numel() + skip.numel() + out.numel())):
            ya = _ARENA.slot(out.device) if needs_amax() else None     # lastconv's x_amax, without a pass of its own
            rc = lib.dsm_spp_concat(_p(raw), _p(skip), _p(br), _p(out), B, H, W, _p(ya), _stream())
        _lib.check(rc, "dsm_spp_concat")
    if ya is not None:
        out._dsm_amax = ya
    return out


# ----------------------------------------------------------------------------
# Conv3d / ConvTranspose3d (k=3) with autograd: training through the 3-D trunk
# ----------------------------------------------------------------------------
def _wgrad_precision(x, g, mode=None):
    """(precision, x_amax, g_amax) of a weight-gradient launch in ``mode`` (None: the ``conv_precision`` option)."""
    mode = _mode(mode)
    if mode not in ("f16x2", "f16"):
        return _lib.DSM_PREC_F32, None, None
    return (_lib.DSM_PREC_F16X2 if mode == "f16x2" else _lib.DSM_PREC_F16), amax_of(x), amax_of(g)


def _wgrad(x_cl, g_cl, cx, cg, stride):
    """dW[g][c][tap] = sum_v X[v*stride + tap - 1][c] G[v][g]  ->  (cg, cx, 3, 3, 3)."""
    B = x_cl.shape[0]
    ws = torch.empty((cx // 32) * (cg // 32) * 27 * 1024, device=x_cl.device, dtype=torch.float32)
    dw = torch.empty((cg, cx, 3, 3, 3), device=x_cl.device, dtype=torch.float32)
    prec, xa, ga = _wgrad_precision(x_cl, g_cl)
    with torch.cuda.device(x_cl.device), _timed("conv3d_wgrad_%s_kernel<S=%d,%dx%d>" % (_OPTIONS["conv_precision"], stride, cx, cg),
                                                54.0 * cx * cg * B * g_cl.shape[2] * g_cl.shape[3] * g_cl.shape[4]):
        rc = _lib.load().dsm_conv3d_wgrad(_p(x_cl), _p(g_cl), _p(ws), _p(dw), B, cx, cg,
                                          x_cl.shape[2], x_cl.shape[3], x_cl.shape[4],
                                          g_cl.shape[2], g_cl.shape[3], g_cl.shape[4], stride,
                                          _conv_flags(), prec, _p(xa), _p(ga), _stream())
    _lib.check(rc, "dsm_conv3d_wgrad")
    return dw


class Conv3dFunction(torch.autograd.Function):
    """y = conv(x, weight) (+ bias) with k = 3, padding 1: ``nn.Conv3d(stride 1|2)`` or
    ``nn.ConvTranspose3d(stride 2, output_padding 1)`` -- forward and both gradients on the
    gfx950 kernels.  bwd-data is a convolution with re-packed weights on the forward kernels;
    bwd-weight is ``dsm_conv3d_wgrad``.  In the reference this is autograd through nn.Conv3d."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, transposed):
        _require_device("Conv3dFunction", x, weight, bias)
        x = carry_amax(to_channels_last_3d(x), x)
        cout = weight.shape[1] if transposed else weight.shape[0]
        packed = pack_conv3d_weight(weight, transposed)
        shift = None if bias is None else bias.detach().contiguous()
        scale = None if bias is None else torch.ones_like(shift)
        y = conv3d_block(x, packed, cout, scale, shift, None, stride, transposed, 0)
        ctx.save_for_backward(x, weight)
        ctx.cfg = (stride, transposed, bias is not None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        stride, transposed, has_bias = ctx.cfg
        gy = carry_amax(to_channels_last_3d(gy), gy)
        if needs_amax():
            amax_of(x), amax_of(gy)             # one pass each at most, shared by bwd-data and bwd-weight
        B, cin = x.shape[0], x.shape[1]
        cout = gy.shape[1]
        dx = dw = db = None
        w = weight.detach()
        if cout == 1 and transposed:                    # GCNet's head l37: ConvTranspose3d(C -> 1, s2)
            dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
            dw = torch.empty_like(w) if ctx.needs_input_grad[1] else None
            with torch.cuda.device(x.device):
                rc = _lib.load().dsm_deconv3d_cout1_bwd(
                    _p(x), _p(gy), _p(w.contiguous()), _p(dx), _p(dw), B, cin, x.shape[2],
                    x.shape[3], x.shape[4], gy.shape[2], gy.shape[3], gy.shape[4], _stream())
            _lib.check(rc, "dsm_deconv3d_cout1_bwd")
        elif cout == 1 and stride != 1:
            raise NotImplementedError("Conv3dFunction.backward: a stride-%d convolution to one "
                                      "channel is not a layer of the reference" % stride)
        elif cout == 1:                                 # classifier head, stride 1, not transposed
            packed = pack_conv3d_weight(w, False)       # [27][Cin]
            dwt = torch.empty(27 * cin, device=x.device, dtype=torch.float32)
            dx = torch.empty_like(x)
            with torch.cuda.device(x.device):
                rc = _lib.load().dsm_conv3d_cout1_bwd(
                    _p(x), _p(gy), _p(packed), _p(dx) if ctx.needs_input_grad[0] else None,
                    _p(dwt) if ctx.needs_input_grad[1] else None, B, cin, x.shape[2], x.shape[3],
                    x.shape[4], _stream())
            _lib.check(rc, "dsm_conv3d_cout1_bwd")
            if not ctx.needs_input_grad[0]:
                dx = None
            if ctx.needs_input_grad[1]:
                dw = dwt.view(27, cin).t().contiguous().view(1, cin, 3, 3, 3)
        else:
            if ctx.needs_input_grad[0]:
                if transposed:                          # dX = conv_s2(dY, W as (out=Cin, in=Cout))
                    dx = conv3d_block(gy, pack_conv3d_weight(w, False), cin, stride=2,
                                      out_size=x.shape[2:])
                elif stride == 1:                       # dX = conv_s1(dY, flipped W^T)
                    wt = w.flip(2, 3, 4).transpose(0, 1).contiguous()
                    dx = conv3d_block(gy, pack_conv3d_weight(wt, False), cin, stride=1)
                else:                                   # dX = convT_s2(dY, W), cropped to x
                    dx = conv3d_block(gy, pack_conv3d_weight(w, True), cin, stride=2,
                                      transposed=True, out_size=x.shape[2:])
                if tuple(dx.shape) != tuple(x.shape):
                    raise RuntimeError("Conv3dFunction.backward: dX shape %s != %s"
                                       % (tuple(dx.shape), tuple(x.shape)))
            if ctx.needs_input_grad[1]:
                if transposed:                          # roles swapped: X := dY, G := x
                    dw = _wgrad(gy, x, cout, cin, 2)    # (Cin, Cout, 3,3,3)
                else:
                    dw = _wgrad(x, gy, cin, cout, stride)
        if has_bias and ctx.needs_input_grad[2]:
            db = gy.sum(dim=(0, 2, 3, 4))
        return dx, dw, db, None, None


def conv3d(x, weight, bias=None, stride=1, transposed=False):
    return Conv3dFunction.apply(x, weight, bias, int(stride), bool(transposed))


# ----------------------------------------------------------------------------
# train-mode BatchNorm3d + cropped skip add + ReLU, fused (csrc/bn3d.hip)
# ----------------------------------------------------------------------------
class BnAddRelu3dFunction(torch.autograd.Function):
    """out = relu?( batch_norm(y; batch statistics) (+ residual, cropped to the common corner) )
    for NDHWC fp32 volumes, with explicit backward -- two launches each way instead of the
    reference's nn.BatchNorm3d + myadd_3d + F.relu chain (and their autograd nodes).
    ``relu``: 0 none, 1 after the addition (PSMNet), 2 before it (GCNet).  Running statistics are
    updated in place as nn.BatchNorm3d does."""

    @staticmethod
    def forward(ctx, y, gamma, beta, residual, running_mean, running_var, relu, momentum, eps):
        _require_device("bn_add_relu3d", y, gamma, beta, residual, running_mean, running_var)
        y = to_channels_last_3d(y)
        B, C, Dy, Hy, Wy = y.shape
        a = _lib.Bn3dArgs()
        a.B, a.C, a.Dy, a.Hy, a.Wy = B, C, Dy, Hy, Wy
        oshape = (B, C, Dy, Hy, Wy)
        if residual is not None:
            if residual.shape[0] != B or residual.shape[1] != C:
                raise ValueError("bn_add_relu3d: residual has shape %s" % (tuple(residual.shape),))
            residual = to_channels_last_3d(residual)
            a.Dr, a.Hr, a.Wr = residual.shape[2:]
            oshape = (B, C, min(Dy, a.Dr), min(Hy, a.Hr), min(Wy, a.Wr))
            a.residual = residual.data_ptr()
        out = torch.empty(oshape, device=y.device, dtype=torch.float32, memory_format=_CL3D)
        affine = torch.empty(4 * C, device=y.device, dtype=torch.float32)
        ws = torch.empty(2 * C, device=y.device, dtype=torch.float64)
        a.y, a.out, a.affine, a.workspace = y.data_ptr(), out.data_ptr(), affine.data_ptr(), ws.data_ptr()
        a.gamma = None if gamma is None else gamma.data_ptr()
        a.beta = None if beta is None else beta.data_ptr()
        a.running_mean = None if running_mean is None else running_mean.data_ptr()
        a.running_var = None if running_var is None else running_var.data_ptr()
        a.relu, a.momentum, a.eps = int(relu), float(momentum), float(eps)
        oa = None
        if needs_amax():                               # the next convolution's x_amax, from this epilogue
            oa = _ARENA.slot(y.device)
            a.out_amax = oa.data_ptr()
        with torch.cuda.device(y.device), _timed("bn3d_train_fwd_kernels", 4.0 * (2 * y.numel() + out.numel())):
            rc = _lib.load().dsm_bn3d_train_fwd(ctypes.byref(a), _stream())
        _lib.check(rc, "dsm_bn3d_train_fwd")
        ctx.save_for_backward(y, out if relu == 1 else None, affine)
        ctx.cfg = (int(relu), None if residual is None else tuple(residual.shape), gamma is not None,
                   beta is not None)
        if oa is not None:
            out._dsm_amax = oa
            ctx.out_amax = oa
        return out

    @staticmethod
    def backward(ctx, gout):
        y, out, affine = ctx.saved_tensors
        relu, rshape, has_gamma, has_beta = ctx.cfg
        gout = gout.contiguous(memory_format=_CL3D)
        B, C, Dy, Hy, Wy = y.shape
        a = _lib.Bn3dArgs()
        a.B, a.C, a.Dy, a.Hy, a.Wy = B, C, Dy, Hy, Wy
        dy = torch.empty_like(y, memory_format=_CL3D)
        dres = None
        if rshape is not None:
            a.Dr, a.Hr, a.Wr = rshape[2:]
            if ctx.needs_input_grad[3]:
                dres = torch.empty(rshape, device=y.device, dtype=torch.float32, memory_format=_CL3D)
                a.dresidual = dres.data_ptr()
            else:
                a.residual = y.data_ptr()          # only marks "a residual shaped the output corner"
        ws = torch.empty(2 * C, device=y.device, dtype=torch.float64)
        a.y, a.affine, a.workspace = y.data_ptr(), affine.data_ptr(), ws.data_ptr()
        a.out = None if out is None else out.data_ptr()
        a.gout, a.dy, a.relu = gout.data_ptr(), dy.data_ptr(), relu
        if needs_amax():                               # the maxima of the gradients this node hands on
            dy._dsm_amax = _ARENA.slot(y.device)
            a.dy_amax = dy._dsm_amax.data_ptr()
            if dres is not None:
                dres._dsm_amax = _ARENA.slot(y.device)
                a.dres_amax = dres._dsm_amax.data_ptr()
        with torch.cuda.device(y.device), _timed("bn3d_train_bwd_kernels", 4.0 * (3 * y.numel() + gout.numel())):
            rc = _lib.load().dsm_bn3d_train_bwd(ctypes.byref(a), _stream())
        _lib.check(rc, "dsm_bn3d_train_bwd")
        dbeta = ws[:C].float() if has_beta else None
        dgamma = ws[C:].float() if has_gamma else None
        return dy, dgamma, dbeta, dres, None, None, None, None, None


def bn_add_relu3d(y, gamma, beta, residual, running_mean, running_var, relu, momentum, eps):
    return BnAddRelu3dFunction.apply(y, gamma, beta, residual, running_mean, running_var, int(relu),
                                     float(momentum), float(eps))


def stage_images_nhwc16(left, right=None):
    """The towers' input staging in one launch: (B,C,H,W) image(s), C <= 16, -> (B or 2B, 16, H, W)
    channels_last with zero channels C..15; with ``right`` the two views share the batch
    (left first), as PSMNet's eval forward feeds them."""
    _require_device("stage_images_nhwc16", left, right)
    left = left.contiguous()
    B, C, H, W = left.shape
    if right is not None:
        if tuple(right.shape) != tuple(left.shape):
            raise ValueError("stage_images_nhwc16: the two views differ in shape")
        right = right.contiguous()
    out = torch.empty(((1 if right is None else 2) * B, 16, H, W), device=left.device,
                      dtype=torch.float32, memory_format=_CL2D)
    with torch.cuda.device(left.device):
        rc = _lib.load().dsm_stage_images_nhwc16(_p(left), _p(right), _p(out), B, C, H, W, _stream())
    _lib.check(rc, "dsm_stage_images_nhwc16")
    return out


# ----------------------------------------------------------------------------
# the 2-D towers in training: convolution with explicit gradients, batch-statistics BN
# ----------------------------------------------------------------------------
def conv2d_variant(cout, stride, k, dilation):
    """Is there a kernel for a 1x1 / 3x3 layer of 32 / 64 / 128 outputs in the current precision mode and flags?
    The plan of a stand-in (16 inputs, a 12 x 40 map: no size decides it); wide and 5x5 layers: see blocks2d."""
    if cout not in (32, 64, 128) or k not in (1, 3) or stride < 1 or dilation < 1:
        return False
    return _conv2d_variant(cout, stride, k, dilation, _mode(None), _conv_flags())


@functools.lru_cache(maxsize=None)
def _conv2d_variant(cout, stride, k, dilation, mode, flags):      # memoised: fused_ok asks per layer and forward
    return _conv_plan(_conv2d_standin(1, 16, cout, 12, 40, stride, k, dilation, mode, flags))[0] == _lib.DSM_OK


def _wgrad2d(x_cl, g_cl, stride, dilation, label="conv2d_wgrad_kernel", mode=None):
    """dW[g][c][ky][kx] = sum_v X[v*stride + (k - 1)*dilation][c] G[v][g]  ->  (cg, cx, 3, 3)."""
    B, cx, Hx, Wx = x_cl.shape
    _, cg, Hg, Wg = g_cl.shape
    ws = torch.empty((cx // 32) * (cg // 32) * 9 * 1024, device=x_cl.device, dtype=torch.float32)
    dw = torch.empty((cg, cx, 3, 3), device=x_cl.device, dtype=torch.float32)
    prec, xa, ga = _wgrad_precision(x_cl, g_cl, mode)
    with torch.cuda.device(x_cl.device), _timed(label, 18.0 * cx * cg * B * Hg * Wg):
        rc = _lib.load().dsm_conv2d_wgrad(_p(x_cl), _p(g_cl), _p(ws), _p(dw), B, cx, cg, Hx, Wx,
                                          Hg, Wg, int(stride), int(dilation), _conv_flags(mode), prec,
                                          _p(xa), _p(ga), _stream())
    _lib.check(rc, "dsm_conv2d_wgrad")
    return dw


class Conv2dFunction(torch.autograd.Function):
    """y = conv2d(x, weight), k in {1, 3}, padding = dilation * (k // 2), no bias: the ``nn.Conv2d`` of
    ``convbn`` (models/psmnet/submodule.py:10-13) with the forward, bwd-data (a convolution again,
    flipped transposed weights) and bwd-weight (``dsm_conv2d_wgrad``; 1x1: one GEMM) on the gfx950
    kernels, NHWC.  Gradients no kernel here covers (stride-2 bwd-data, the 3-channel image layer's
    bwd-weight, channel counts outside the compiled variants) come from
    ``aten.convolution_backward`` on the same tensors.  In the reference this is autograd through
    nn.Conv2d."""

    @staticmethod
    def forward(ctx, x, weight, stride, dilation):
        _require_device("Conv2dFunction", x, weight)
        cout, cin, k, _ = weight.shape
        x = x.contiguous(memory_format=_CL2D)
        xs = x
        if cin % 16:                                   # the image: 3 -> 16 staged channels
            xs = torch.zeros((x.shape[0], (cin + 15) // 16 * 16) + tuple(x.shape[2:]), device=x.device,
                             dtype=x.dtype).contiguous(memory_format=_CL2D)
            xs[:, :cin] = x
        packed = pack_conv2d_weight(weight, xs.shape[1])
        y = conv2d_block(xs, packed, cout, stride=stride, k=k, dilation=dilation)
        ctx.save_for_backward(x, weight)
        ctx.cfg = (int(stride), int(dilation))
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        stride, dil = ctx.cfg
        cout, cin, k, _ = weight.shape
        gy = gy.contiguous(memory_format=_CL2D)
        w = weight.detach()
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dx = dw = None
        if need_dx and stride == 1 and conv2d_variant(cin, 1, k, dil) and cout % 16 == 0:
            wt = (w.flip(2, 3) if k == 3 else w).transpose(0, 1).contiguous()
            dx = conv2d_block(gy, pack_conv2d_weight(wt), cin, stride=1, k=k, dilation=dil)
        if need_dw and k == 3 and cin % 32 == 0 and cout % 32 == 0:
            dw = _wgrad2d(x, gy, stride, dil)
        elif need_dw and k == 1:
            xg = x if stride == 1 else x[:, :, ::stride, ::stride]
            dw = torch.matmul(gy.permute(0, 2, 3, 1).reshape(-1, cout).t(),
                              xg.permute(0, 2, 3, 1).reshape(-1, cin)).view(cout, cin, 1, 1)
        mask = [need_dx and dx is None, need_dw and dw is None, False]
        if mask[0] or mask[1]:
            pad = dil * (k // 2)
            rdx, rdw, _ = torch.ops.aten.convolution_backward(
                gy, x, w, None, [stride, stride], [pad, pad], [dil, dil], False, [0, 0], 1, mask)
            dx = rdx if mask[0] else dx
            dw = rdw if mask[1] else dw
        return dx, dw, None, None


def conv2d(x, weight, stride=1, dilation=1):
    return Conv2dFunction.apply(x, weight, int(stride), int(dilation))


# ----------------------------------------------------------------------------
# training through the wide 3x3 layers (DispNetC conv3b .. conv6b, iResNet conv3_1 .. conv6_1)
# ----------------------------------------------------------------------------
# Forward and gradient packs of a wide layer's weight, made once per weight version: DispNetC's forward runs
# twice per self-supervised step on the same weights, and both backwards need the flipped / transposed
# pack.  Keyed like blocks2d._Folded2d (storage address, ``_version``, the epoch that a hipGraph replay
# advances); an entry is replaced when its weight changes and dropped with the weight.
_WIDE_PACKS = {}
_WIDE_PACK_MISSES = {"forward": 0, "gradient": 0}      # packs made so far (tests count them)


def _wide_pack_entry(weight):
    key = _versions(weight)
    ent = _WIDE_PACKS.get(id(weight))
    if ent is None or ent["ref"]() is not weight:
        weakref.finalize(weight, _WIDE_PACKS.pop, id(weight), None)
        ent = None
    if ent is None or ent["key"] != key:
        ent = {"ref": weakref.ref(weight), "key": key, "forward": None, "gradient": None}
        _WIDE_PACKS[id(weight)] = ent
    return ent


def _wide_pack(ent, weight, which):
    if ent[which] is None:
        w = weight.detach()
        if which == "gradient":                        # backward-data: a convolution with flipped W^T
            w = w.flip(2, 3).transpose(0, 1).contiguous()
        ent[which] = pack_conv2d_weight(w)
        _WIDE_PACK_MISSES[which] += 1
    return ent[which]


class WideConv2dReLUFunction(torch.autograd.Function):
    """y = relu(conv2d(x, weight, k3, pad 1, stride 1 | 2) + bias) for Cin and Cout in 256 / 512 / 1024, NHWC,
    every pass on the gfx950 kernels (fp16 precision modes): the wide MFMA kernel forward;
    ``dsm_bias_relu_bwd`` for the masked gradient, the bias gradient and the gradient's maximum;
    backward-data on the wide kernel again (stride 1: flipped transposed weights; stride 2: its transposed
    mode); ``dsm_conv2d_wgrad`` for the weight gradient.  No device value is read on the host and the
    workspaces come from torch's allocator per call, so a step captures into a hipGraph.  The backward runs in
    the precision mode of its forward, whatever ``conv_precision`` says by then.  In the reference
    this is autograd through ``conv2d_bn(..., bn=False)`` (models/util_conv.py:100-117)."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride):
        _require_device("WideConv2dReLUFunction", x, weight, bias)
        cout, cin, k, k2 = weight.shape
        if k != 3 or k2 != 3 or cin not in WIDE2D_COUT or cout not in WIDE2D_COUT or stride not in (1, 2):
            raise ValueError("wide_conv2d_relu: no kernels for weight %s at stride %s"
                             % (tuple(weight.shape), stride))
        if bias is None:
            raise ValueError("wide_conv2d_relu: the layer has a bias")
        if not x.is_contiguous(memory_format=_CL2D):
            x = carry_amax(x.contiguous(memory_format=_CL2D), x)
        ent = _wide_pack_entry(weight)
        y = conv2d_block(x, _wide_pack(ent, weight, "forward"), cout, None, bias.detach().contiguous(),
                         stride=stride, relu=1)
        ctx.save_for_backward(x, weight, y)
        ctx.stride, ctx.packs, ctx.mode = int(stride), ent, _OPTIONS["conv_precision"]
        # the maxima ride on the tensor objects; kept here too for a saved tensor that comes back as another
        # object.  ``amax_of`` checks their generation and replaces a stale one by a fresh pass.
        ctx.amax = (getattr(x, "_dsm_amax", None), getattr(y, "_dsm_amax", None))
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, y = ctx.saved_tensors
        mode = ctx.mode                                # the mode the saved maxima and the forward belong to
        for t, slot in zip((x, y), ctx.amax):
            if slot is not None and getattr(t, "_dsm_amax", None) is None:
                t._dsm_amax = slot
        stride = ctx.stride
        cout, cin = weight.shape[0], weight.shape[1]
        need_dx, need_dw, need_db = ctx.needs_input_grad[:3]
        g, db = bias_relu_bwd(gy, y, need_db, mode=mode)
        dx = dw = None
        if need_dx:
            packed = _wide_pack(ctx.packs, weight, "gradient")
            if stride == 1:
                dx = conv2d_block(g, packed, cin, stride=1, mode=mode)
            else:
                dx = conv2d_transposed_block(g, packed, cin, x.shape[2:], mode=mode)
        if need_dw:
            dw = _wgrad2d(x, g, stride, 1, "conv2d_wgrad_kernel<S=%d,%dx%d>" % (stride, cin, cout), mode=mode)
        return dx, dw, db, None


def wide_conv2d_relu(x, weight, bias, stride=1):
    return WideConv2dReLUFunction.apply(x, weight, bias, int(stride))


def bn_add_relu2d(y, gamma, beta, residual, running_mean, running_var, relu, momentum, eps):
    """Train-mode BatchNorm2d (+ skip add) (+ ReLU) on NHWC maps: the 3-D kernels on (B, C, 1, H, W)
    views of the same memory."""
    y = y.contiguous(memory_format=_CL2D).unsqueeze(2)
    if residual is not None:
        residual = residual.contiguous(memory_format=_CL2D).unsqueeze(2)
    return bn_add_relu3d(y, gamma, beta, residual, running_mean, running_var, relu, momentum,
                         eps).squeeze(2)


# ----------------------------------------------------------------------------
# decoder level of DispNetC / iResNet: deconv bias + ReLU + x2 upsampling + myCat2d, one launch
# ----------------------------------------------------------------------------
def decoder_level(deconv, x, pr, skip):
    """``myCat2d(deconv(x), upsample(pr), skip)`` of the reference's decoders
    (models/dispnetcorr.py:89-132, models/iresnet.py:119-161,186-193; util_fun.py:7-15) with
    ``deconv`` = ``Sequential(ConvTranspose2d(bias), ReLU)`` or a bare ``ConvTranspose2d``.
    Eval mode on the GPU: the transposed convolution runs without its bias (stock kernel) and ONE
    launch does bias + ReLU + bilinear x2 upsampling of ``pr`` + the crops + the concatenation;
    under autograd the same with the option ``decoder_train`` on (``DecoderCatFunction``: the transposed
    convolution stays a stock autograd node); otherwise (training, autograd, CPU) the stock ops."""
    import torch.nn as nn
    import torch.nn.functional as F
    conv = deconv[0] if isinstance(deconv, nn.Sequential) else deconv
    relu = isinstance(deconv, nn.Sequential) and len(deconv) > 1
    fast = (x.is_cuda and (not torch.is_grad_enabled() or _OPTIONS["decoder_train"]) and
            x.dtype == torch.float32 and isinstance(conv, nn.ConvTranspose2d) and
            (not relu or (len(deconv) == 2 and isinstance(deconv[1], nn.ReLU))))
    if not fast:
        seq = [deconv(x)]
        if pr is not None:
            seq.append(F.interpolate(pr, scale_factor=2, mode="bilinear", align_corners=False))
        if skip is not None:
            seq.append(skip)
        h = min(t.shape[2] for t in seq)
        w = min(t.shape[3] for t in seq)
        return torch.cat([t[:, :, :h, :w] for t in seq], dim=1)
    up = F.conv_transpose2d(x, conv.weight, None, conv.stride, conv.padding, conv.output_padding,
                            conv.groups, conv.dilation).contiguous()
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (up, conv.bias, pr, skip)):
        return DecoderCatFunction.apply(up, conv.bias, pr, skip, bool(relu))
    return _decoder_cat_fwd(up, conv.bias, pr, skip, relu)


def _decoder_cat_fwd(up, bias, pr, skip, relu):
    B, Cu, Hu, Wu = up.shape
    pr = None if pr is None else pr.contiguous()
    skip = None if skip is None else skip.contiguous()
    Cp, Hp, Wp = (0, 0, 0) if pr is None else pr.shape[1:]
    Cs, Hs, Ws = (0, 0, 0) if skip is None else skip.shape[1:]
    h = min([Hu] + ([2 * Hp] if Cp else []) + ([Hs] if Cs else []))
    w = min([Wu] + ([2 * Wp] if Cp else []) + ([Ws] if Cs else []))
    out = torch.empty((B, Cu + Cp + Cs, h, w), device=up.device, dtype=torch.float32)
    with torch.cuda.device(up.device), _timed("decoder_cat_kernel", 8.0 * out.numel()):
        rc = _lib.load().dsm_decoder_cat(_p(up), _p(bias), _p(pr), _p(skip), _p(out), B, Cu, Cp, Cs,
                                         Hu, Wu, Hp, Wp, Hs, Ws, int(relu), _stream())
    _lib.check(rc, "dsm_decoder_cat")
    return out


class DecoderCatFunction(torch.autograd.Function):
    """``relu?(up + bias) | upsample_x2(pr) | skip`` of ``decoder_level`` under autograd: ``up`` is the stock
    transposed convolution's output without its bias.  Only the output is saved (the following ``iconv`` keeps
    it anyway): its first ``Cu`` channels are the ReLU mask.  The backward is one call of
    ``dsm_decoder_cat_bwd``; ``g_bias`` is the only gradient summed with atomics."""

    @staticmethod
    def forward(ctx, up, bias, pr, skip, relu):
        out = _decoder_cat_fwd(up.contiguous(), bias, pr, skip, relu)
        ctx.relu = bool(relu)
        ctx.shapes = (tuple(up.shape), None if pr is None else tuple(pr.shape),
                      None if skip is None else tuple(skip.shape))
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, g):
        out, = ctx.saved_tensors
        su, sp, ss = ctx.shapes
        need_up, need_b, need_pr, need_skip = ctx.needs_input_grad[:4]
        B, Cu, Hu, Wu = su
        Cp, Hp, Wp = (0, 0, 0) if sp is None else sp[1:]
        Cs, Hs, Ws = (0, 0, 0) if ss is None else ss[1:]
        g = g.contiguous()

        def new(shape, need):
            return torch.empty(shape, device=g.device, dtype=torch.float32) if need else None
        g_up, g_b = new(su, need_up), new((Cu,), need_b)
        g_pr, g_skip = new(sp, need_pr and Cp > 0), new(ss, need_skip and Cs > 0)
        work = 4.0 * sum(t.numel() for t in (g_up, g_pr, g_skip) if t is not None) * 2 + \
            (4.0 * B * Cu * out.shape[2] * out.shape[3] if ctx.relu else 0.0)
        with torch.cuda.device(g.device), _timed("decoder_cat_bwd_kernel", work):
            rc = _lib.load().dsm_decoder_cat_bwd(_p(g), _p(out), _p(g_up), _p(g_b), _p(g_pr), _p(g_skip),
                                                 B, Cu, Cp, Cs, Hu, Wu, Hp, Wp, Hs, Ws, int(ctx.relu), _stream())
        _lib.check(rc, "dsm_decoder_cat_bwd")
        return g_up, g_b, g_pr, g_skip, None


# ----------------------------------------------------------------------------
# Self-supervised depthmono[-mask], Cap[_ds][_lr][-mask] and common[-mask] pyramid loss (csrc/selfsup.hip)
# ----------------------------------------------------------------------------
_SELFSUP_TERMS = {"ds": _lib.DSM_SELFSUP_DS, "lr": _lib.DSM_SELFSUP_LR}


def _selfsup_flags(spec):
    """The flags word of dsm_selfsup_fwd / _bwd and the ``_timed`` label suffix of the objective."""
    flags = _lib.DSM_SELFSUP_MASK if spec["flag_mask"] else 0
    if spec["objective"] == "depthmono":
        return flags, ""
    if spec["objective"] == "common":                # dsm_selfsup_ext_* (the older entry points refuse the word)
        return flags | _lib.DSM_SELFSUP_COMMON, "_common"
    if spec["objective"] == "sssmnet":
        return flags | _lib.DSM_SELFSUP_SSSMNET, "_sssmnet"
    flags |= _lib.DSM_SELFSUP_CAP
    for t in spec["terms"]:
        flags |= _SELFSUP_TERMS[t]
    return flags, "_cap" + "".join("_" + t for t in ("ds", "lr") if t in spec["terms"])


def _int_strides(name, t):
    st = t.stride()
    if any(s < 0 or s >= 2 ** 31 for s in st) or t.numel() >= 2 ** 31:
        raise ValueError("%s: strides %s do not fit the kernel's 32-bit indexing" % (name, st))
    return st


def _selfsup_view_scalars(dl, side, objective):
    """(delt_im, delt_disp, delt_im1) of view ``side`` (0 left, 1 flipped) of one pyramid entry from
    its epsilons ``dl`` in the reference's draw order: imL_wrap, imL1_wrap, dispL_wrap, dispL1_wrap
    -- for SsSMnet imL_wrap, imL1_wrap, imL_wrap1, imL1_wrap1[, dispL_wrap, dispL1_wrap].  A
    disparity epsilon the name does not draw is 0, as is delt_im1 outside SsSMnet.  The ONE place
    that knows this order: the items, the side array and ``selfsup_step_params`` all ask here."""
    sss = objective == "sssmnet"
    dd = 2 + side + (2 if sss else 0)
    return (float(dl[side]), float(dl[dd]) if dd < len(dl) else 0.0, float(dl[2 + side]) if sss else 0.0)


def _selfsup_n_delts(objective, flag_mask):
    return 6 if objective == "sssmnet" and flag_mask else 4


def selfsup_step_params(delts, weights, objective="depthmono", flag_mask=True, out=None):
    """The (2n, 4) float32 CPU tensor that ``selfsup_pyramid_loss(..., params=)`` reads on the device:
    row 2p + side = [delt_im, delt_disp, delt_im1, weight] of view ``side`` of entry p
    (include/dsmnet_hip.h, dsm_selfsup_dyn_*).  ``delts[p]``: the entry's epsilons in the reference's
    draw order (four; six for SsSMnet with ``flag_mask``), ``weights[p]`` its level weight.  ``out``:
    filled and returned when given (e.g. a pinned buffer)."""
    n = len(delts)
    if len(weights) != n or n < 1:
        raise ValueError("selfsup_step_params: one weight per epsilon set")
    n_delts = _selfsup_n_delts(objective, flag_mask)
    if any(len(dl) != n_delts for dl in delts):
        raise ValueError("selfsup_step_params: %s%s takes %d epsilons per entry"
                         % (objective, "-mask" if flag_mask else "", n_delts))
    rows = [_selfsup_view_scalars(delts[p], side, objective) + (float(weights[p]),)
            for p in range(n) for side in range(2)]
    if out is None:
        return torch.tensor(rows, dtype=torch.float32)
    if out.device.type != "cpu" or out.dtype != torch.float32 or tuple(out.shape) != (2 * n, 4) or not out.is_contiguous():
        raise ValueError("selfsup_step_params: out must be a contiguous float32 CPU tensor (%d, 4)" % (2 * n))
    out.copy_(torch.tensor(rows, dtype=torch.float32))
    return out


class SelfsupPyramidLossFunction(torch.autograd.Function):
    """Items 2p / 2p+1 = the two views of pyramid entry p (csrc/selfsup.hip).  ``spec`` holds the
    host-side description; the tensors ride as arguments so that autograd sees the disparities.
    ``spec["params"]``: the device array of the per-step scalars (dsm_selfsup_dyn_*), or None."""

    @staticmethod
    def _items(spec, imgs, disps, grads=None):
        imL, imR_src, imL1, imR1_src = imgs
        n = len(spec["levels"])
        items = (_lib.SelfsupItem * (2 * n))()
        for p in range(n):
            k, sf = spec["levels"][p], spec["factors"][p]
            dL, dL1 = disps[p], disps[n + p]
            gL, gL1 = (grads[p], grads[n + p]) if grads is not None else (None, None)
            for side, (im, src, lt, d, do, g, go) in enumerate((
                    (imL, imR_src, spec["lefttop"], dL, dL1, gL, gL1),
                    (imL1, imR1_src, spec["lefttop1"], dL1, dL, gL1, gL))):
                lvl = im[:, :, ::2 ** k, ::2 ** k]
                it = items[2 * p + side]
                it.im, it.src = lvl.data_ptr(), src.data_ptr()
                it.disp, it.disp_other = d.data_ptr(), do.data_ptr()
                it.grad_disp = None if g is None else g.data_ptr()
                it.grad_other = None if go is None else go.data_ptr()
                it.im_stride[:] = list(lvl.stride())
                it.src_stride[:] = list(src.stride())
                it.B, it.h, it.w = lvl.shape[0], lvl.shape[2], lvl.shape[3]
                it.H0, it.W0 = src.shape[2], src.shape[3]
                it.left, it.top = int(lt[0]), int(lt[1])
                it.scale_factor = int(sf)
                if spec["params"] is None:               # else the kernels read them from the device array
                    it.delt_im, it.delt_disp, _ = _selfsup_view_scalars(spec["delts"][p], side, spec["objective"])
                    it.weight = float(spec["weights"][p])
                it.ds_divisor = int(spec["ds_divisors"][p])
        return items

    @staticmethod
    def _ext(spec, disps, warp, gwarp=None):
        """SsSMnet's side array: item 2p + side owns the (B,3,h,w) slices of ``warp`` / ``gwarp`` at
        three times the offset of its disparity in the flat gradient buffer."""
        n = len(spec["levels"])
        ext = (_lib.SelfsupExt * (2 * n))()
        offs, o = [], 0
        for d in disps:
            offs.append(o)
            o += 3 * d.numel()
        for p in range(n):
            for side in range(2):
                e = ext[2 * p + side]
                at = 4 * offs[side * n + p]
                e.warp = warp.data_ptr() + at
                e.grad_warp = None if gwarp is None else gwarp.data_ptr() + at
                if spec["params"] is None:
                    e.delt_im1 = _selfsup_view_scalars(spec["delts"][p], side, spec["objective"])[2]
        return ext

    @staticmethod
    def forward(ctx, spec, imL, imR_src, imL1, imR1_src, *disps):
        imgs = (imL, imR_src, imL1, imR1_src)
        items = SelfsupPyramidLossFunction._items(spec, imgs, disps)
        lib = _lib.load()
        flags, tag = _selfsup_flags(spec)
        sss = bool(flags & _lib.DSM_SELFSUP_SSSMNET)
        ext = sss or bool(flags & _lib.DSM_SELFSUP_COMMON)
        nf = (lib.dsm_selfsup_ext_workspace_floats(items, len(items), flags) if ext
              else lib.dsm_selfsup_workspace_floats(items, len(items)))
        if nf == 0:
            raise ValueError("selfsup_pyramid_loss: empty or invalid item list")
        ws = torch.empty(nf, device=imL.device, dtype=torch.float32)
        loss = torch.empty((), device=imL.device, dtype=torch.float32)
        aux = torch.empty(4 * len(items), device=imL.device, dtype=torch.float32)
        # every objective enters the library once; depthmono keeps the label under which its timings
        # are on record, the others name their kernels "+"-joined, as suploss's does
        label = "selfsup%s_fwd%s" % (tag, ("_warp+tiles+reduce" if sss else "_gradmean+tiles+reduce" if ext
                                           else "_tiles+reduce") if tag else "")
        # SsSMnet: every item's im_wrap, written by the first launch, kept for the backward
        warp = torch.empty(3 * sum(d.numel() for d in disps) if sss else 0, device=imL.device, dtype=torch.float32)
        params = spec["params"]
        with torch.cuda.device(imL.device), _timed(label, 4.0 * (nf + warp.numel())):
            side = SelfsupPyramidLossFunction._ext(spec, disps, warp) if sss else None
            if params is not None:
                rc = lib.dsm_selfsup_dyn_fwd(items, side, len(items), flags, _p(params), _p(ws), _p(loss), _p(aux), _stream())
            elif ext:
                rc = lib.dsm_selfsup_ext_fwd(items, side, len(items), flags, _p(ws), _p(loss), _p(aux), _stream())
            else:
                rc = lib.dsm_selfsup_fwd(items, len(items), flags, _p(ws), _p(loss), _p(aux), _stream())
        _lib.check(rc, "dsm_selfsup_dyn_fwd" if params is not None else "dsm_selfsup_ext_fwd" if ext else "dsm_selfsup_fwd")
        ctx.spec = spec
        ctx.save_for_backward(imL, imR_src, imL1, imR1_src, ws, aux, warp, *disps)
        ctx.mark_non_differentiable(aux)
        return loss, aux

    @staticmethod
    def backward(ctx, gloss, gaux):
        saved = ctx.saved_tensors
        imgs, ws, aux, warp, disps = saved[:4], saved[4], saved[5], saved[6], saved[7:]
        flags, tag = _selfsup_flags(ctx.spec)
        # with the lr term the kernel accumulates (the other view scatters in); without it every
        # element is stored by its one writer, so the buffer needs no fill launch
        scatter = not (flags & _lib.DSM_SELFSUP_CAP) or bool(flags & _lib.DSM_SELFSUP_LR)
        sss = bool(flags & _lib.DSM_SELFSUP_SSSMNET)
        nd = sum(d.numel() for d in disps)
        # SsSMnet: the scatter goes into a zeroed (B,3,h,w) buffer per item, which shares the one fill
        # with the gradient buffer
        flat = (torch.zeros if scatter else torch.empty)(nd + warp.numel(), device=ws.device, dtype=torch.float32)
        grads, o = [], 0
        for d in disps:
            grads.append(flat[o:o + d.numel()].view(d.shape))
            o += d.numel()
        items = SelfsupPyramidLossFunction._items(ctx.spec, imgs, disps, grads)
        g = gloss.to(torch.float32).contiguous()
        label = "selfsup%s_bwd%s" % (tag, "_tiles+chain" if sss else "" if scatter else "_gather")
        ext = sss or bool(flags & _lib.DSM_SELFSUP_COMMON)
        params = ctx.spec["params"]      # kept by the spec: the array the forward read, read again now
        with torch.cuda.device(ws.device), _timed(label, 4.0 * (ws.numel() + 2 * flat.numel())):
            side = SelfsupPyramidLossFunction._ext(ctx.spec, disps, warp, flat[nd:]) if sss else None
            if params is not None:
                rc = _lib.load().dsm_selfsup_dyn_bwd(items, side, len(items), flags, _p(params), _p(ws), _p(aux), _p(g), _stream())
            elif ext:
                rc = _lib.load().dsm_selfsup_ext_bwd(items, side, len(items), flags, _p(ws), _p(aux), _p(g), _stream())
            else:
                rc = _lib.load().dsm_selfsup_bwd(items, len(items), flags, _p(ws), _p(aux), _p(g), _stream())
        _lib.check(rc, "dsm_selfsup_dyn_bwd" if params is not None else "dsm_selfsup_ext_bwd" if ext else "dsm_selfsup_bwd")
        return (None, None, None, None, None) + tuple(grads)


def selfsup_pyramid_loss(imL, imR_src, lefttop, dispLs, imL1, imR1_src, lefttop1, dispL1s, levels,
                         weights, factors, flag_mask, delts, return_aux=False, objective="depthmono",
                         terms=("ds", "lr"), ds_divisors=None, params=None):
    """The reference's depthmono[-mask] objective over a disparity pyramid in two launches forward
    (tiles, reduce) and two backward (the gradient buffer's fill, tiles) (csrc/selfsup.hip; losses/loss.py:196-236, 393-405, 424-467,
    losses/SSIM.py, utils/imwrap.py:37-72):

        sum_p weights[p] * (loss_depthmono(imL_k, imwrap(imR_src, dispLs[p], LeftTop=lefttop,
                scale_factor=factors[p]), dispLs[p], imwrap(dispL1s[p], dispLs[p], fliplr=True))
              + the same for the flipped view)

    with imL_k = imL[:, :, ::2**k, ::2**k], k = levels[p].  ``imL``/``imL1`` (B,3,h,w) and
    ``imR_src``/``imR1_src`` (B,3,H0,W0) may be strided views; ``dispLs[p]``/``dispL1s[p]``
    (B,1,h_k,w_k) take the gradient.  ``delts[p]`` = the reference's four random epsilons of the
    entry, in its draw order (imL_wrap, imL1_wrap, dispL_wrap, dispL1_wrap).  No host
    synchronisation.  ``return_aux``: also the (2P,4) per-view [w, fallback, C, simlary].

    ``objective="cap"``: loss_Cap_ds_lr (loss.py:238-283) in place of loss_depthmono -- no
    "< 1024 valid pixels" fallback (no valid pixel: w = 0.001), the terms named in ``terms`` (any
    of "ds", "lr") only, and the smoothness term weighted w / ``ds_divisors[p]`` (positive
    integers; None: 1).  The forward is the same two launches.  Without "lr" the backward is ONE
    gather launch into an unfilled buffer and the gradient is bit-reproducible; with it, the fill
    and the scatter of depthmono.  depthmono always has
    both terms and no divisor: ``terms`` and ``ds_divisors`` must be left at their defaults.

    ``objective="common"``: loss_common (loss.py:154-194) -- depthmono's rule in everything (the
    fallback, both terms, the masks, w_ds = w_lr = w, four epsilons) with the depth-ratio
    smoothness C_ds3 (loss.py:99-114) in place of C_ds1: on d = |disp| + 1,
    |d[i]/d[i+1] + d[i]/d[i-1] - 2| clamped to [0, 10], weighted by
    exp(-max_c |diff1(im)| / (0.5 m)) with m the mean of |diff1(im)| over (C,H,W) of each batch
    sample, x and y apart.  One more forward launch sums those means in a fixed order (loss and
    aux stay bit-identical from run to run); the backward is depthmono's fill and scatter.
    ``terms`` and ``ds_divisors`` must be left at their defaults.

    ``objective="sssmnet"``: loss_SsSMnet through losses_pyramid2 (loss.py:285-324, 469-512) -- per
    view C_ap = mean(0.425(1-ssim) + 0.15(|im-im_wrap| + C_imdiff1(im, im_wrap))), C_lr =
    mean|im - im_wrap1| with im_wrap1 the OTHER view's im_wrap warped again by this view's
    disparity (fliplr), C_ds = mean C_ds2(im, disp) weighted w / ``ds_divisors[p]``, 1e-4 mean|disp|;
    w from the mean SSIM over mask_ap with no fallback (no valid pixel: w = 0.001).  ``delts[p]``:
    imL_wrap, imL1_wrap, imL_wrap1, imL1_wrap1 and, with ``flag_mask`` only, dispL_wrap, dispL1_wrap
    (4 or 6 values).  Forward 3 launches (every im_wrap, tiles, reduce); backward the fill and 2: the
    tiles scatter d C_lr / d im_wrap into the other view's zeroed buffer, a second launch chains it
    to the disparity.  ``terms`` must be left at its default.

    ``params``: the per-step scalars from DEVICE memory instead of ``weights`` / ``delts`` (both must
    then be None) -- a float32 tensor (2n, 4) on the images' device, contiguous and 16-byte aligned,
    laid out as ``selfsup_step_params`` builds it.  The kernels read it when they run
    (dsm_selfsup_dyn_fwd / _bwd, the same kernels), so a captured graph replays with whatever the
    array holds at that moment; the function keeps the tensor for its backward, and its contents
    must not change between the forward and the backward of one step.  Same values, same loss bits
    as the host-argument form."""
    n = len(dispLs)
    if params is not None:
        if weights is not None or delts is not None:
            raise ValueError("selfsup_pyramid_loss: with params, weights and delts must be None")
        if not (torch.is_tensor(params) and params.dtype == torch.float32 and tuple(params.shape) == (2 * n, 4)
                and params.is_contiguous() and params.device == imL.device and params.data_ptr() % 16 == 0):
            raise ValueError("selfsup_pyramid_loss: params must be a contiguous, 16-byte aligned float32 tensor "
                             "(%d, 4) on %s" % (2 * n, imL.device))
    elif weights is None or delts is None:
        raise ValueError("selfsup_pyramid_loss: weights and delts, or params")
    if objective not in ("depthmono", "cap", "common", "sssmnet"):
        raise ValueError("selfsup_pyramid_loss: objective %r is none of 'depthmono', 'cap', 'common', 'sssmnet'"
                         % (objective,))
    terms = tuple(terms)
    if any(t not in _SELFSUP_TERMS for t in terms):
        raise ValueError("selfsup_pyramid_loss: terms %r: only 'ds' and 'lr' exist" % (terms,))
    if objective != "cap" and set(terms) != {"ds", "lr"}:
        raise ValueError("selfsup_pyramid_loss: %s has both terms: leave ``terms`` at its default" % objective)
    if objective in ("depthmono", "common") and ds_divisors is not None:
        raise ValueError("selfsup_pyramid_loss: %s has both terms and no ds_divisors" % objective)
    if ds_divisors is None:
        ds_divisors = [1] * n
    if len(ds_divisors) != n or any(int(v) != v or int(v) < 1 for v in ds_divisors):
        raise ValueError("selfsup_pyramid_loss: ds_divisors %r: one integer >= 1 per disparity" % (ds_divisors,))
    if weights is None:
        if not (len(dispL1s) == len(levels) == len(factors) == n) or n < 1:
            raise ValueError("selfsup_pyramid_loss: one level and factor per disparity")
    elif not (len(dispL1s) == len(levels) == len(weights) == len(factors) == len(delts) == n) or n < 1:
        raise ValueError("selfsup_pyramid_loss: one level, weight, factor and delt set per disparity")
    if 2 * n > 16:
        raise ValueError("selfsup_pyramid_loss: at most 8 pyramid entries, got %d" % n)
    n_delts = _selfsup_n_delts(objective, flag_mask)
    if delts is not None and any(len(dl) != n_delts for dl in delts):
        raise ValueError("selfsup_pyramid_loss: %s%s takes %s epsilons per entry"
                         % (objective, "-mask" if flag_mask else "", "six" if n_delts == 6 else "four"))
    _require_device("selfsup_pyramid_loss", imL, imR_src, imL1, imR1_src, *dispLs, *dispL1s)
    dev = imL.device
    for t in (imR_src, imL1, imR1_src) + tuple(dispLs) + tuple(dispL1s):
        if t.device != dev:
            raise ValueError("selfsup_pyramid_loss: every tensor must be on %s, got %s" % (dev, t.device))
    for name, im, src in (("imL", imL, imR_src), ("imL1", imL1, imR1_src)):
        if im.dim() != 4 or im.shape[1] != 3 or src.dim() != 4 or src.shape[:2] != im.shape[:2]:
            raise ValueError("selfsup_pyramid_loss: %s %s and its source %s must be (B,3,h,w) and "
                             "(B,3,H0,W0)" % (name, tuple(im.shape), tuple(src.shape)))
        if min(src.shape[2:]) <= 1:
            raise ValueError("selfsup_pyramid_loss: maps must be larger than 1x1")   # imwrap.py:48
        _int_strides(name, im)
        _int_strides(name, src)
    if imL.shape != imL1.shape:
        raise ValueError("selfsup_pyramid_loss: the two views differ: %s vs %s"
                         % (tuple(imL.shape), tuple(imL1.shape)))
    B, _, h, w = imL.shape
    ds = []
    for p in range(n):
        k = int(levels[p])
        hk, wk = -(-h // 2 ** k), -(-w // 2 ** k)
        for d in (dispLs[p], dispL1s[p]):
            if tuple(d.shape) != (B, 1, hk, wk):
                # the reference would fail to broadcast im against disp here
                raise ValueError("selfsup_pyramid_loss: disparity %d is %s, its image level %d is %s"
                                 % (p, tuple(d.shape), k, (B, 1, hk, wk)))
            if hk <= 1 or wk <= 1:
                raise ValueError("selfsup_pyramid_loss: maps must be larger than 1x1")
        if int(factors[p]) < 1:
            raise ValueError("selfsup_pyramid_loss: bad factor at entry %d" % p)
    ds = [d.contiguous() for d in dispLs] + [d.contiguous() for d in dispL1s]
    spec = {"levels": [int(k) for k in levels], "factors": [int(f) for f in factors],
            "weights": None if weights is None else [float(x) for x in weights],
            "delts": None if delts is None else [tuple(float(x) for x in dl) for dl in delts], "params": params,
            "lefttop": (int(lefttop[0]), int(lefttop[1])), "lefttop1": (int(lefttop1[0]), int(lefttop1[1])),
            "flag_mask": bool(flag_mask), "objective": objective, "terms": terms,
            "ds_divisors": [int(v) for v in ds_divisors]}
    loss, aux = SelfsupPyramidLossFunction.apply(spec, imL, imR_src, imL1, imR1_src, *ds)
    return (loss, aux.view(2 * n, 4)) if return_aux else loss


# ----------------------------------------------------------------------------
# Supervised pyramid loss with D1 / EPE (csrc/suploss.hip)
# ----------------------------------------------------------------------------
def supervised_loss_supported(disp_gt, disps, levels):
    """True when ``supervised_pyramid_loss`` takes these maps: everything CUDA fp32 on one device,
    gt (B,1,H,W), every prediction (B,[1,]hc,wc) with hc * 2^level >= H and wc * 2^level >= W (the
    reference's crop then yields the full H x W), at most 16 of them."""
    if not (torch.is_tensor(disp_gt) and disp_gt.is_cuda and disp_gt.dtype == torch.float32 and disp_gt.dim() == 4
            and disp_gt.shape[1] == 1 and disp_gt.numel() > 0):
        return False
    if not 1 <= len(disps) <= _lib.DSM_SUPLOSS_MAX_ITEMS or len(levels) != len(disps):
        return False
    B, _, H, W = disp_gt.shape
    for d, k in zip(disps, levels):
        if not (d.is_cuda and d.dtype == torch.float32 and d.device == disp_gt.device and 0 <= int(k) <= 12):
            return False
        if d.dim() == 4 and d.shape[1] != 1 or d.dim() not in (3, 4) or d.shape[0] != B or d.numel() == 0:
            return False
        if (d.shape[-2] << int(k)) < H or (d.shape[-1] << int(k)) < W:
            return False
    return True


class SupervisedPyramidLossFunction(torch.autograd.Function):
    """``spec`` = (levels, weights, flag_smooth); gt and the (B,1,hc,wc) predictions ride as
    arguments so that autograd sees the predictions."""

    @staticmethod
    def _items(spec, disps, grads=None):
        items = (_lib.SuplossItem * len(disps))()
        for i, d in enumerate(disps):
            it = items[i]
            it.pred = d.data_ptr()
            it.grad = None if grads is None or grads[i] is None else grads[i].data_ptr()
            it.B, it.hc, it.wc = d.shape[0], d.shape[2], d.shape[3]
            it.level, it.weight = spec[0][i], spec[1][i]
        return items

    @staticmethod
    def forward(ctx, spec, gt, *disps):
        B, _, H, W = gt.shape
        n = len(disps)
        save = any(ctx.needs_input_grad[2:])
        items = SupervisedPyramidLossFunction._items(spec, disps)
        lib = _lib.load()
        nf = lib.dsm_suploss_workspace_floats(n, B, H, W, int(save))
        if nf == 0:
            raise ValueError("supervised_pyramid_loss: empty or invalid item list")
        ws = torch.empty(nf, device=gt.device, dtype=torch.float32)
        loss = torch.empty((), device=gt.device, dtype=torch.float32)
        aux = torch.empty(1 + 4 * n, device=gt.device, dtype=torch.float32)
        coarse = sum(d.numel() for d in disps)
        with torch.cuda.device(gt.device), _timed("suploss_fwd_tiles+reduce", 4.0 * (n * gt.numel() + coarse + nf)):
            rc = lib.dsm_suploss_fwd(items, n, _p(gt), H, W, int(spec[2]), int(save), _p(ws), _p(loss),
                                     _p(aux), _stream())
        _lib.check(rc, "dsm_suploss_fwd")
        ctx.spec = spec
        ctx.save_for_backward(gt, ws, aux, *disps)
        ctx.mark_non_differentiable(aux)
        return loss, aux

    @staticmethod
    def backward(ctx, gloss, gaux):
        saved = ctx.saved_tensors
        gt, ws, aux, disps = saved[0], saved[1], saved[2], saved[3:]
        grads = [torch.empty_like(d) if need else None for d, need in zip(disps, ctx.needs_input_grad[2:])]
        items = SupervisedPyramidLossFunction._items(ctx.spec, disps, grads)
        g = gloss.to(torch.float32).contiguous()
        B, _, H, W = gt.shape
        work = 4.0 * (sum(gt.numel() + d.numel() for d, gr in zip(disps, grads) if gr is not None))
        with torch.cuda.device(gt.device), _timed("suploss_bwd_gather", work):
            rc = _lib.load().dsm_suploss_bwd(items, len(items), _p(gt), H, W, int(ctx.spec[2]), _p(ws),
                                             _p(aux), _p(g), _stream())
        _lib.check(rc, "dsm_suploss_bwd")
        return (None, None) + tuple(grads)


def supervised_pyramid_loss(disp_gt, disps, levels, weights, flag_smooth=True):
    """The reference's supervised objective over a pyramid of outputs, and its accuracy metrics, in
    two launches forward and one backward (csrc/suploss.hip; losses/loss.py:326-338, 407-421,
    stereo.py:103-113):

        loss = sum_i weights[i] * loss_supervised(disp_gt, upsample(disps[i], 2**levels[i])[:, :, :H, :W],
                                                  flag_smooth)

    ``disp_gt`` (B,1,H,W); ``disps[i]`` (B,1,hc,wc) or (B,hc,wc) with hc * 2**levels[i] >= H and
    wc * 2**levels[i] >= W (``supervised_loss_supported``); at most 16 outputs.  Returns
    ``(loss, metrics)``: ``metrics`` is the (1 + 4 * len(disps),) device tensor n, then per output
    L1 mean, smooth mean, EPE and D1 %.  No valid pixel (n == 0): loss 0 with zero gradients, EPE and
    D1 NaN.  No host synchronisation."""
    n = len(disps)
    if n < 1 or not (len(levels) == len(weights) == n):
        raise ValueError("supervised_pyramid_loss: one level and one weight per prediction")
    _require_device("supervised_pyramid_loss", disp_gt, *disps)
    if n > _lib.DSM_SUPLOSS_MAX_ITEMS:
        raise ValueError("supervised_pyramid_loss: at most %d predictions, got %d" % (_lib.DSM_SUPLOSS_MAX_ITEMS, n))
    if not supervised_loss_supported(disp_gt, disps, levels):
        raise ValueError("supervised_pyramid_loss: gt %s with predictions %s at levels %s is not supported "
                         "(gt (B,1,H,W); every upsampled prediction must cover it)"
                         % (tuple(disp_gt.shape), [tuple(d.shape) for d in disps], list(levels)))
    ds = [(d.unsqueeze(1) if d.dim() == 3 else d).contiguous() for d in disps]
    spec = ([int(k) for k in levels], [float(w) for w in weights], bool(flag_smooth))
    loss, aux = SupervisedPyramidLossFunction.apply(spec, disp_gt.contiguous(), *ds)
    return loss, aux


# ----------------------------------------------------------------------------
# Stereo colour augmentation (csrc/color.hip)
# ----------------------------------------------------------------------------
def stereo_color(x, records, alpha, groups):
    """Rewrite the (B,C,H,W) batch ``x`` IN PLACE with the fused colour steps of
    myTransforms.Stereo_color / Stereo_normalize (csrc/color.hip; myTransforms/aug_color.py:28-45,
    66-101, 103-203).  ``records``: B*groups tuples ``(order, jitter, flags, alpha_row)``, record
    b*groups + g for channels 3g..3g+2 of image b (``dsmnet_amd.transforms`` draws them);
    ``alpha``: the (B,groups,3) device tensor of Lighting's draws (None when no record lights).
    One launch per 64 records, on the current stream, no host synchronisation.  Returns ``x``."""
    if not x.is_cuda:
        _require_device("stereo_color", x)
    if x.dtype != torch.float32:
        raise ValueError("stereo_color: x must be float32, got %s" % x.dtype)
    if x.dim() != 4 or x.shape[1] < 6:
        raise ValueError("stereo_color: x must be (B, C >= 6, H, W), got %s" % (tuple(x.shape),))
    if not x.is_contiguous():
        raise ValueError("stereo_color: x must be a dense NCHW tensor (not a strided view)")
    if groups not in (1, 2):
        raise ValueError("stereo_color: groups must be 1 or 2, got %r" % (groups,))
    B, C, H, W = x.shape
    if len(records) != B * groups:
        raise ValueError("stereo_color: %d records for %d images x %d groups" % (len(records), B, groups))
    recs = (_lib.ColorRecord * len(records))()
    lights = False
    for r, (order, jitter, flags, row) in zip(recs, records):
        r.order[:] = [int(o) for o in order]
        r.jitter[:] = [float(j) for j in jitter]
        r.flags, r.alpha_row = int(flags), int(row)
        lights = lights or bool(r.flags & _lib.DSM_COLOR_LIGHTING)
    if lights:
        if alpha is None:
            raise ValueError("stereo_color: Lighting records need the alpha tensor")
        _require_device("stereo_color", alpha)
        if alpha.device != x.device or not alpha.is_contiguous() or alpha.numel() < 3 * B * groups:
            raise ValueError("stereo_color: alpha must be a dense (B, groups, 3) tensor on %s" % x.device)
    with torch.cuda.device(x.device), _timed("stereo_color_kernel", 8.0 * B * 3 * groups * H * W):
        rc = _lib.load().dsm_stereo_color(_p(x), _p(alpha) if lights else None, recs, len(records),
                                          B, C, H, W, groups, _stream())
    _lib.check(rc, "dsm_stereo_color")
    return x


# ----------------------------------------------------------------------------
# Stereo spatial augmentation + ToTensor (csrc/spatial.hip)
# ----------------------------------------------------------------------------
def stereo_spatial(x, records, out_hw, to_tensor_channels=6):
    """The (B,C,h,w) training batch of the (B,H0,W0,C) channels-last frames ``x`` (imL | imR
    [| dispL [| dispR]], 6 <= C <= 8): myTransforms.Spatial_stereo's shift, crop and optional
    linear resize, then ToTensor_numpy's transpose and / 255 of the first ``to_tensor_channels``
    (0 or 6) planes (csrc/spatial.hip; myTransforms/aug_spatial.py:7-88, aug_color.py:15-26).
    ``records``: B tuples ``(shift, ws, hs, w, h, resize, scale_rand, scale_x, scale_y)``, the
    source window in the shifted frame (``dsmnet_amd.transforms`` draws them); ``out_hw`` =
    (h, w) of the output.  ``x`` is not modified.  One launch per 48 records, on the current
    stream, no host synchronisation.  Returns the new batch."""
    if not x.is_cuda:
        _require_device("stereo_spatial", x)
    if x.dtype != torch.float32:
        raise ValueError("stereo_spatial: x must be float32, got %s" % x.dtype)
    if x.dim() != 4 or not 6 <= x.shape[3] <= 8:
        raise ValueError("stereo_spatial: x must be (B, H0, W0, C) channels last with 6 <= C <= 8, got %s"
                         % (tuple(x.shape),))
    if not x.is_contiguous():
        raise ValueError("stereo_spatial: x must be a dense (B, H0, W0, C) tensor (not a strided view)")
    if to_tensor_channels not in (0, 6):
        raise ValueError("stereo_spatial: to_tensor_channels must be 0 or 6, got %r" % (to_tensor_channels,))
    B, H0, W0, C = x.shape
    h, w = int(out_hw[0]), int(out_hw[1])
    if B < 1 or h < 1 or w < 1:
        raise ValueError("stereo_spatial: empty batch or output (B = %d, out_hw = %s)" % (B, (h, w)))
    if len(records) != B:
        raise ValueError("stereo_spatial: %d records for %d images" % (len(records), B))
    recs = (_lib.SpatialRecord * B)()
    for r, (shift, ws, hs, rw, rh, resize, scale_rand, scale_x, scale_y) in zip(recs, records):
        r.shift, r.ws, r.hs, r.w, r.h = int(shift), int(ws), int(hs), int(rw), int(rh)
        r.resize, r.scale_rand = int(bool(resize)), float(scale_rand)
        r.scale_x, r.scale_y = float(scale_x), float(scale_y)
    y = torch.empty(B, C, h, w, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device), _timed("stereo_spatial_kernel", 8.0 * B * C * h * w):
        rc = _lib.load().dsm_stereo_spatial(_p(x), _p(y), recs, B, B, C, H0, W0, h, w,
                                            int(to_tensor_channels), _stream())
    _lib.check(rc, "dsm_stereo_spatial")
    return y


_DISP_BYTES = {_lib.DSM_DISP_F32: 4, _lib.DSM_DISP_U16_256: 2, _lib.DSM_DISP_U16: 2, _lib.DSM_DISP_U8: 1}


def stereo_spatial_raw(raw, sources, records, frame_hw, C, out_hw, to_tensor_channels=6):
    """``stereo_spatial`` from the decoded files' bytes: the (B,C,h,w) training batch of B samples
    whose planes lie in the 1-D uint8 device tensor ``raw`` as decoded -- (Hs,Ws,3) uint8 RGB,
    (Hs,Ws) uint8 / uint16 / float32 disparity -- without forming the fp32 frames (csrc/frames.hip;
    myDatasets_stereo/Dataset_stereo.py:63-74, 86-99, 121-123, then aug_spatial.py:7-88 and
    aug_color.py:15-26).  ``sources``: B tuples ``(imL, imR, dispL, dispR, Hs, Ws, y0, x0, flip,
    disp_format)`` in the field order of ``dsm_frame_source`` (byte offsets into ``raw``, -1 for an
    absent disparity; ``disp_format`` one of ``_lib.DSM_DISP_*``): frame pixel (y, x) of the
    ``frame_hw`` = (H0, W0) frame is source pixel (y0 + y, x0 + (W0 - 1 - x if flip else x)).
    ``records``, ``out_hw`` and ``to_tensor_channels`` as for ``stereo_spatial``, and the result is
    bit-identical to it on frames assembled on the host.  One launch per 32 images, on the current
    stream, no host synchronisation.  Returns the new batch."""
    if not raw.is_cuda:
        _require_device("stereo_spatial_raw", raw)
    if raw.dtype != torch.uint8 or raw.dim() != 1 or not raw.is_contiguous():
        raise ValueError("stereo_spatial_raw: raw must be a dense 1-D uint8 tensor, got %s %s"
                         % (raw.dtype, tuple(raw.shape)))
    C = int(C)
    if not 6 <= C <= 8:
        raise ValueError("stereo_spatial_raw: 6 <= C <= 8 (imL | imR [| dispL [| dispR]]), got %d" % C)
    if to_tensor_channels not in (0, 6):
        raise ValueError("stereo_spatial_raw: to_tensor_channels must be 0 or 6, got %r" % (to_tensor_channels,))
    B = len(sources)
    H0, W0 = int(frame_hw[0]), int(frame_hw[1])
    h, w = int(out_hw[0]), int(out_hw[1])
    if B < 1 or H0 < 1 or W0 < 1 or h < 1 or w < 1:
        raise ValueError("stereo_spatial_raw: empty batch, frame or output (B = %d, frame_hw = %s, out_hw = %s)"
                         % (B, (H0, W0), (h, w)))
    if len(records) != B:
        raise ValueError("stereo_spatial_raw: %d records for %d images" % (len(records), B))
    srcs = (_lib.FrameSource * B)()
    nbytes = 0
    for s, (imL, imR, dispL, dispR, Hs, Ws, y0, x0, flip, disp_format) in zip(srcs, sources):
        s.imL, s.imR, s.dispL, s.dispR = int(imL), int(imR), int(dispL), int(dispR)
        s.Hs, s.Ws, s.y0, s.x0 = int(Hs), int(Ws), int(y0), int(x0)
        s.flip, s.disp_format = int(flip), int(disp_format)
        nbytes += 6 + (C - 6) * _DISP_BYTES.get(s.disp_format, 0)
    recs = (_lib.SpatialRecord * B)()
    for r, (shift, ws, hs, rw, rh, resize, scale_rand, scale_x, scale_y) in zip(recs, records):
        r.shift, r.ws, r.hs, r.w, r.h = int(shift), int(ws), int(hs), int(rw), int(rh)
        r.resize, r.scale_rand = int(bool(resize)), float(scale_rand)
        r.scale_x, r.scale_y = float(scale_x), float(scale_y)
    y = torch.empty(B, C, h, w, device=raw.device, dtype=torch.float32)
    lib = _lib.load()
    step = _lib.DSM_FRAMES_MAX_RECORDS
    with torch.cuda.device(raw.device):
        # validate the whole batch before the first launch: a refused call leaves y untouched
        _lib.check(lib.dsm_stereo_spatial_raw_plan(_p(raw), raw.numel(), srcs, _p(y), recs, B, B, C, H0, W0, h, w,
                                                   int(to_tensor_channels)), "dsm_stereo_spatial_raw")
        for b0 in range(0, B, step):
            nb = min(step, B - b0)
            yb = y[b0:b0 + nb]
            with _timed("stereo_spatial_raw_kernel", (float(nbytes) / B + 4.0 * C) * nb * h * w):
                rc = lib.dsm_stereo_spatial_raw(
                    _p(raw), raw.numel(), ctypes.cast(ctypes.byref(srcs, b0 * ctypes.sizeof(_lib.FrameSource)),
                                                      ctypes.POINTER(_lib.FrameSource)), _p(yb),
                    ctypes.cast(ctypes.byref(recs, b0 * ctypes.sizeof(_lib.SpatialRecord)),
                                ctypes.POINTER(_lib.SpatialRecord)), nb, nb, C, H0, W0, h, w,
                    int(to_tensor_channels), _stream())
            _lib.check(rc, "dsm_stereo_spatial_raw")
    return y


# ----------------------------------------------------------------------------
# Evaluation metrics: D1 / EPE, the KITTI set, photometric error (csrc/metrics.hip)
# ----------------------------------------------------------------------------
METRIC_KEYS = ("d1", "epe", "abs_rel", "sq_rel", "rmse", "rmse_log", "d1_kitti", "a1", "a2", "a3",
               "pixelerror", "pixelerror_elem")


def stereo_metrics(pred, gt=None, imL=None, imR=None, delt=None, negate_warp=False):
    """The sums behind every evaluation number of utils/evaluate.py (``evaluate``,
    ``imwrap_pixel_errors``, ``compute_errors``) and stereo.py:103-113 ``accuracy``, in two launches
    and without a host read (csrc/metrics.hip; the 16 slots are listed in include/dsmnet_hip.h and
    DESIGN.md).  ``pred`` (B,1,H,W) or (B,H,W); ``gt`` (B,1,H,W) with holes <= 0, or None; ``imL`` /
    ``imR`` (B,C,H,W), both or neither, warped as ``imwrap_BCHW(imR, pred)`` -- ``negate_warp=True``
    samples at ``-pred``, as evaluate.py:26,40 do.  ``delt``: the warp's epsilon (None: one draw of
    ``train._draw_delt()``, from the CPU generator).  The ``> 0`` masks of the photometric slots mean
    "inside the right image" only for non-negative images (raw [0,1], not normalised ones).

    Returns the (B,16) float64 device tensor of per-image sums; ``stereo_metrics_finish`` turns it
    into the metrics.  The rows are additive: summing them over images, batches or ranks and then
    finishing gives the metrics of the union.  Capturable: torch allocates, nothing synchronises."""
    _require_device("stereo_metrics", pred, gt, imL, imR)
    if pred.dim() == 3:
        pred = pred.unsqueeze(1)
    if pred.dim() != 4 or pred.shape[1] != 1 or pred.numel() == 0:
        raise ValueError("stereo_metrics: pred must be (B,1,H,W) or (B,H,W), got %s" % (tuple(pred.shape),))
    B, _, H, W = pred.shape
    if gt is None and imL is None and imR is None:
        raise ValueError("stereo_metrics: give gt, or imL and imR, or all three")
    if (imL is None) != (imR is None):
        raise ValueError("stereo_metrics: imL and imR come together")
    if gt is not None and tuple(gt.shape) != (B, 1, H, W):
        raise ValueError("stereo_metrics: gt %s does not match pred %s" % (tuple(gt.shape), tuple(pred.shape)))
    C = 1
    if imL is not None:
        C = imL.shape[1] if imL.dim() == 4 else 0
        if C < 1 or tuple(imL.shape) != (B, C, H, W) or imR.shape != imL.shape:
            raise ValueError("stereo_metrics: imL %s and imR %s must both be (B,C,H,W) over pred %s"
                             % (tuple(imL.shape), tuple(imR.shape), tuple(pred.shape)))
        if min(H, W) < 2:
            raise ValueError("stereo_metrics: maps must be larger than 1x1")        # imwrap.py:48
        if delt is None:
            from . import train
            delt = train._draw_delt()
    lib = _lib.load()
    a = _lib.MetricsArgs()
    keep = [t if t is None else t.contiguous() for t in (pred, gt, imL, imR)]
    ws = torch.empty(lib.dsm_stereo_metrics_workspace_bytes(B, H, W) // 8, device=pred.device, dtype=torch.float64)
    out = torch.empty((B, _lib.DSM_METRICS_SLOTS), device=pred.device, dtype=torch.float64)
    a.pred, a.gt, a.imL, a.imR = [None if t is None else t.data_ptr() for t in keep]
    a.workspace, a.out = ws.data_ptr(), out.data_ptr()
    a.B, a.C, a.H, a.W = B, C, H, W
    a.delt = float(delt or 0.0)
    a.flags = _lib.DSM_METRICS_NEGATE_WARP if negate_warp else 0
    work = 4.0 * B * H * W * (1 + (gt is not None) + (2 * C if imL is not None else 0)) + 8.0 * ws.numel()
    with torch.cuda.device(pred.device), _timed("metrics_tiles+reduce", work):
        rc = lib.dsm_stereo_metrics(ctypes.byref(a), _stream())
    _lib.check(rc, "dsm_stereo_metrics")
    out.image_shape = (C, H, W) if imL is not None else None
    return out


def stereo_metrics_finish(sums, per_image=False, image_shape=None):
    """The metrics of a (B,16) tensor of ``stereo_metrics`` sums: plain torch on any device, no host
    read.  Returns a dict of float64 tensors, 0-dim over the whole batch or (B,) with ``per_image``:

        d1, epe                       evaluate / accuracy: 100 - 100 * good / n, mean |gt - pred|
        abs_rel, sq_rel, rmse, rmse_log, d1_kitti, a1, a2, a3      compute_errors
        pixelerror                    evaluate: 255 * mean |imL - w| over the pixels whose warped
                                      channel sum is > 0; over every element when there is none
        pixelerror_elem               imwrap_pixel_errors: 255 * mean over the elements with w > 0

    ``image_shape`` = (C, H, W) of the images, which ``pixelerror`` needs; by default what
    ``stereo_metrics`` noted on its result (``sums.image_shape``; sums combined from several results
    have lost it: pass it).  Without it ``pixelerror`` is NaN.  No valid ground-truth pixel (n = 0,
    or no gt given) makes the ground-truth metrics NaN, as numpy's empty means are; no element with
    w > 0 makes ``pixelerror_elem`` NaN."""
    if sums.dim() != 2 or sums.shape[1] != _lib.DSM_METRICS_SLOTS:
        raise ValueError("stereo_metrics_finish: sums must be (B,16), got %s" % (tuple(sums.shape),))
    if image_shape is None:
        image_shape = getattr(sums, "image_shape", None)
    nimg = sums.shape[0]
    s = sums.to(torch.float64)
    s = s if per_image else s.sum(0)
    c = [s[..., k] for k in range(_lib.DSM_METRICS_SLOTS)]
    n = c[0]
    mean = s[..., :11] / n.unsqueeze(-1)                 # every ground-truth slot over n, one launch
    pct = 100.0 * mean[..., 2:4]
    root = torch.sqrt(mean[..., 4:6])
    out = {"d1": 100.0 - pct[..., 0], "epe": mean[..., 1], "abs_rel": mean[..., 6], "sq_rel": mean[..., 7],
           "rmse": root[..., 0], "rmse_log": root[..., 1], "d1_kitti": pct[..., 1],
           "a1": mean[..., 8], "a2": mean[..., 9], "a3": mean[..., 10]}
    if image_shape is None:
        out["pixelerror"] = torch.full_like(n, float("nan"))
    else:
        C, H, W = image_shape
        every = float((1 if per_image else nimg) * C * H * W)
        inside = c[13] > 0
        out["pixelerror"] = 255.0 * torch.where(inside, c[14] / (C * torch.where(inside, c[13], torch.ones_like(n))),
                                                c[15] / every)
    out["pixelerror_elem"] = 255.0 * c[12] / c[11]
    return out


# ----------------------------------------------------------------------------
# Left-right check and background fill of a predicted map (csrc/lrcheck.hip)
# ----------------------------------------------------------------------------
LRCheck = collections.namedtuple("LRCheck", ("wrap", "weight", "mask", "masked"))


def _plane_maps(name, *maps):
    """(B,1,H,W) or (B,H,W) float32 device maps of one shape -> detached contiguous tensors, (B,H,W)."""
    shape = tuple(maps[0].shape)
    if len(shape) == 4 and shape[1] == 1:
        B, H, W = shape[0], shape[2], shape[3]
    elif len(shape) == 3:
        B, H, W = shape
    else:
        raise ValueError("%s: a map is (B,1,H,W) or (B,H,W), got %s" % (name, shape))
    for m in maps[1:]:
        if tuple(m.shape) != shape:
            raise ValueError("%s: shapes differ: %s vs %s" % (name, tuple(m.shape), shape))
    if min(B, H, W) < 1:
        raise ValueError("%s: empty map %s" % (name, shape))
    return [m.detach().contiguous() for m in maps], (B, H, W)


def lr_check(disp, other, mirrored=True, delt=0.0, factor=1.0, threshold=1.0,
             want=("wrap", "weight", "mask", "masked")):
    """Left-right consistency of ``disp`` against the other view's map, in one launch and without a
    host read (csrc/lrcheck.hip, ``dsm_lr_check``): ``wrap = imwrap_BCHW(other, disp, fliplr=True)``
    (utils/imwrap.py:37-72 as loss.py:451-452 call it), ``weight = weight_common(disp, wrap, factor)``
    (loss.py:393-404), ``mask = (|disp - wrap| / factor < threshold) & (the sample lies inside the
    image)`` as ``torch.bool`` and ``masked = disp * mask``.

    ``disp`` / ``other``: (B,1,H,W) or PSMNet's (B,H,W), float32, the same shape; the results have it
    too.  ``mirrored=True``: ``other`` was predicted from the mirrored, swapped pair and is still in
    that frame (what the -mask objectives hand to the warp).  ``mirrored=False``: ``other`` is the
    right camera's map in its own frame (``gcnet_LR``'s second output, what ``deploy --flip``
    writes); it is read mirrored, without a copy, and the result is bit-identical to
    ``lr_check(disp, other.flip(-1))``.  The right view's own check is the same call with the roles
    swapped, in the mirrored frame.  ``delt``: the reference's warp epsilon; 0 (inference) makes the
    result deterministic.  ``want``: the entries to compute; the others are None.

    No autograd backward: the inputs are detached.  Capturable: torch allocates, nothing synchronises."""
    _require_device("lr_check", disp, other)
    names = tuple(want)
    if not names or any(n not in LRCheck._fields for n in names):
        raise ValueError("lr_check: want is a non-empty subset of %s, got %r" % (LRCheck._fields, want))
    (d, o), (B, H, W) = _plane_maps("lr_check", disp, other)
    if min(H, W) < 2:
        raise ValueError("lr_check: maps must be larger than 1x1")                   # imwrap.py:48
    out = {n: torch.empty(disp.shape, device=disp.device, dtype=torch.uint8 if n == "mask" else torch.float32)
           for n in names}
    a = _lib.LrcheckArgs()
    a.disp, a.other = d.data_ptr(), o.data_ptr()
    for n in names:
        setattr(a, n, out[n].data_ptr())
    a.B, a.H, a.W = B, H, W
    a.delt, a.factor, a.threshold = float(delt), float(factor), float(threshold)
    a.flags = 0 if mirrored else _lib.DSM_LRCHECK_OTHER_RIGHT_FRAME
    work = B * H * W * (8.0 + sum(1.0 if n == "mask" else 4.0 for n in names))
    with torch.cuda.device(disp.device), _timed("lr_check_tiles", work):
        rc = _lib.load().dsm_lr_check(ctypes.byref(a), _stream())
    _lib.check(rc, "dsm_lr_check")
    if "mask" in out:
        out["mask"] = out["mask"].view(torch.bool)          # the kernel writes 0 / 1
    return LRCheck(*[out.get(n) for n in LRCheck._fields])


def fill_background(disp, mask):
    """``disp`` with the pixels ``mask`` rejects filled from the background, in two launches and
    without a host read (csrc/lrcheck.hip, ``dsm_fill_background``): an invalid pixel gets the smaller
    of the nearest valid values to its left and right in its row (the one that exists at a border),
    a row without a valid pixel the element-wise smaller of the nearest filled rows above and below,
    an image without a valid pixel zeros.  Valid pixels are unchanged; the value of an invalid pixel
    is never read, so a NaN there cannot spread.  ``disp`` (B,1,H,W) or (B,H,W) float32, ``mask`` the
    same shape, ``torch.bool`` or ``torch.uint8``.  Returns a new tensor of ``disp``'s shape.  No
    autograd backward; capturable."""
    _require_device("fill_background", disp)
    if not mask.is_cuda:
        _require_device("fill_background", mask)
    if mask.dtype not in (torch.bool, torch.uint8):
        raise TypeError("fill_background: mask is torch.bool or torch.uint8, got %s" % (mask.dtype,))
    if mask.shape != disp.shape:
        raise ValueError("fill_background: mask %s does not match disp %s" % (tuple(mask.shape), tuple(disp.shape)))
    (d, m), (B, H, W) = _plane_maps("fill_background", disp, mask)
    lib = _lib.load()
    out = torch.empty(disp.shape, device=disp.device, dtype=torch.float32)
    ws = torch.empty(lib.dsm_fill_background_workspace_bytes(B, H, W) // 4, device=disp.device, dtype=torch.int32)
    with torch.cuda.device(disp.device), _timed("fill_rows+empty_rows", 14.0 * B * H * W):
        rc = lib.dsm_fill_background(_p(d), _p(m), _p(out), _p(ws), B, H, W, _stream())
    _lib.check(rc, "dsm_fill_background")
    return out


# ----------------------------------------------------------------------------
# Speckle filter of a predicted map: connected regions, the small ones removed (csrc/speckle.hip)
# ----------------------------------------------------------------------------
Speckle = collections.namedtuple("Speckle", ("out", "keep", "size"))


def filter_speckles(disp, max_size, max_diff, valid=None, new_val=0.0, want=("out", "keep")):
    """The connected regions of ``disp`` with the small ones removed, on the device and without a host
    read (csrc/speckle.hip, ``dsm_speckle_filter``): OpenCV's ``filterSpeckles(img, newVal,
    maxSpeckleSize, maxDiff)``, StereoSGBM's ``speckleWindowSize`` / ``speckleRange``.  Exact:

        node    a pixel with ``isfinite(disp)`` that ``valid`` (if given) allows; the value of any other
                pixel is never used, so a NaN there cannot spread
        edge    two 4-neighbours of one image, both nodes, with ``fabsf(disp[p] - disp[q]) <= max_diff``
                in float32; images of a batch are never joined
        region  a connected component (transitive: a ramp of steps <= ``max_diff`` is one region)
        size    ``torch.int32``: the nodes of the pixel's region, 0 where the pixel is no node
        keep    ``torch.bool``: node and ``size > max_size`` -- a region is a speckle iff
                ``size <= max_size``; ``max_size = 0`` removes nothing but the pixels that are no nodes
        out     ``disp`` where ``keep``, else ``new_val``

    ``disp``: (B,1,H,W) or PSMNet's (B,H,W), float32, any H, W >= 1; ``valid`` the same shape,
    ``torch.bool`` or ``torch.uint8`` (``lr_check``'s mask).  ``max_size``: int >= 0; ``max_diff``: finite
    float >= 0.  ``want``: the entries to compute; the others are None.  Returns a ``Speckle`` of new
    tensors of ``disp``'s shape.  Integer atomics only: two runs give the same bits.

    No autograd backward: the inputs are detached.  Capturable: torch allocates (the workspace, 8 bytes per
    pixel, is written before it is read in every call), nothing synchronises, the launches are one chain."""
    names = tuple(want)
    if not names or any(n not in Speckle._fields for n in names) or len(set(names)) != len(names):
        raise ValueError("filter_speckles: want is a non-empty subset of %s, got %r" % (Speckle._fields, want))
    if isinstance(max_size, bool) or int(max_size) != max_size or max_size < 0 or max_size >= 2 ** 31:
        raise ValueError("filter_speckles: max_size is an int >= 0, got %r" % (max_size,))
    if not (0.0 <= float(max_diff) <= 3.402823466e38):
        raise ValueError("filter_speckles: max_diff is finite (in float32) and >= 0, got %r" % (max_diff,))
    if valid is not None:
        if valid.dtype not in (torch.bool, torch.uint8):
            raise TypeError("filter_speckles: valid is torch.bool or torch.uint8, got %s" % (valid.dtype,))
        if valid.shape != disp.shape:
            raise ValueError("filter_speckles: valid %s does not match disp %s" % (tuple(valid.shape), tuple(disp.shape)))
    _require_device("filter_speckles", disp)
    if valid is not None and not valid.is_cuda:
        _require_device("filter_speckles", valid)
    maps, (B, H, W) = _plane_maps("filter_speckles", *[t for t in (disp, valid) if t is not None])
    if B * H * W >= 2 ** 31:
        raise ValueError("filter_speckles: %d pixels are past the kernels' int32 indices" % (B * H * W))
    lib = _lib.load()
    dtypes = {"out": torch.float32, "keep": torch.uint8, "size": torch.int32}
    out = {n: torch.empty(disp.shape, device=disp.device, dtype=dtypes[n]) for n in names}
    ws = torch.empty(lib.dsm_speckle_workspace_bytes(B, H, W) // 4, device=disp.device, dtype=torch.int32)
    a = _lib.SpeckleArgs()
    a.disp, a.valid = maps[0].data_ptr(), None if valid is None else maps[1].data_ptr()
    for n in names:
        setattr(a, n, out[n].data_ptr())
    a.workspace = ws.data_ptr()
    a.B, a.H, a.W = B, H, W
    a.max_size, a.max_diff, a.new_val, a.flags = int(max_size), float(max_diff), float(new_val), 0
    work = B * H * W * (4.0 + (1.0 if valid is not None else 0.0) + 4 * 8.0 +
                        sum(1.0 if n == "keep" else 4.0 for n in names))
    with torch.cuda.device(disp.device), _timed("speckle_label_tiles+merge_borders+flatten_count+apply", work):
        rc = lib.dsm_speckle_filter(ctypes.byref(a), _stream())
    _lib.check(rc, "dsm_speckle_filter")
    if "keep" in out:
        out["keep"] = out["keep"].view(torch.bool)          # the kernel writes 0 / 1
    return Speckle(*[out.get(n) for n in Speckle._fields])


# ----------------------------------------------------------------------------
# Result maps of a predicted map: KITTI 16-bit, 8-bit, viridis, error picture (csrc/encode.hip)
# ----------------------------------------------------------------------------
ENCODE_OUTPUTS = ("u16", "u8", "rgb", "err")


def encode_disparity(disp, gt=None, mask=None, window=None, flip=False, want=("u16",), vrange=None):
    """The bytes of the files a disparity map is kept in, in one launch and without a host read
    (csrc/encode.hip, ``dsm_disp_encode``; the rules per output are in include/dsmnet_hip.h):

        u16   (B,h,w) ``torch.uint16``: KITTI's encoding, ``rint(d * 256)`` in [1, 65535], 0 = invalid
        u8    (B,h,w) ``torch.uint8``: ``clip(rint(d), 0, 255)``, what the reference's ``submit()`` writes
        rgb   (B,h,w,3) ``torch.uint8``: viridis over ``vrange = (lo, hi)``; ``vrange=None`` is
              ``plt.imsave``'s rule, each image over its own finite, unmasked range (one more launch)
        err   (B,h,w,3) ``torch.uint8``: the KITTI devkit's log-scale error picture; needs ``gt``

    ``disp``: (B,1,H,W) or PSMNet's (B,H,W), float32; ``gt`` the same shape, holes <= 0; ``mask`` the same
    shape, ``torch.bool`` or ``torch.uint8``: a pixel it rejects (or whose ``disp`` is not finite) is 0 in
    every output.  ``window = (y0, x0, h, w)``: the part of the frame that is written (default: all of
    it) -- how padding added before the forward is cut off.  ``flip=True`` writes the window mirrored
    (a right view predicted from the mirrored, swapped pair), bit-identical to encoding the flipped
    tensors.  ``want``: a non-empty subset of ``ENCODE_OUTPUTS``.

    Returns a dict of new device tensors.  No autograd; capturable: torch allocates, nothing synchronises."""
    _require_device("encode_disparity", disp, gt)
    names = tuple(want)
    if not names or any(n not in ENCODE_OUTPUTS for n in names) or len(set(names)) != len(names):
        raise ValueError("encode_disparity: want is a non-empty subset of %s, got %r" % (ENCODE_OUTPUTS, want))
    if "err" in names and gt is None:
        raise ValueError("encode_disparity: the error picture needs gt")
    if mask is not None:
        if not mask.is_cuda:
            _require_device("encode_disparity", mask)
        if mask.dtype not in (torch.bool, torch.uint8):
            raise TypeError("encode_disparity: mask is torch.bool or torch.uint8, got %s" % (mask.dtype,))
    maps, (B, Hs, Ws) = _plane_maps("encode_disparity", *[t for t in (disp, gt, mask) if t is not None])
    d = maps[0]
    g = maps[1] if gt is not None else None
    m = maps[-1] if mask is not None else None
    y0, x0, h, w = (0, 0, Hs, Ws) if window is None else [int(v) for v in window]
    if min(h, w) < 1 or y0 < 0 or x0 < 0 or y0 + h > Hs or x0 + w > Ws:
        raise ValueError("encode_disparity: window %r leaves the %dx%d frame" % (tuple(window), Hs, Ws))
    a = _lib.EncodeArgs()
    a.flags = _lib.DSM_ENCODE_FLIP if flip else 0
    if "rgb" in names:
        if vrange is None:
            a.flags |= _lib.DSM_ENCODE_AUTO_RANGE
        else:
            a.vmin, a.vmax = float(vrange[0]), float(vrange[1])
            if not (abs(a.vmin) <= 3.402823466e38 and abs(a.vmax) <= 3.402823466e38 and a.vmax >= a.vmin):
                raise ValueError("encode_disparity: vrange is finite (in float32) with lo <= hi, got %r" % (vrange,))
    lib = _lib.load()
    dev = disp.device
    shapes = {"u16": ((B, h, w), torch.uint16), "u8": ((B, h, w), torch.uint8),
              "rgb": ((B, h, w, 3), torch.uint8), "err": ((B, h, w, 3), torch.uint8)}
    out = {n: torch.empty(shapes[n][0], device=dev, dtype=shapes[n][1]) for n in names}
    ws = None
    if a.flags & _lib.DSM_ENCODE_AUTO_RANGE:
        ws = torch.empty(lib.dsm_disp_encode_workspace_bytes(B, h, w) // 4, device=dev, dtype=torch.float32)
        a.workspace = ws.data_ptr()
    a.disp, a.gt, a.mask = d.data_ptr(), None if g is None else g.data_ptr(), None if m is None else m.data_ptr()
    for n in names:
        setattr(a, n, out[n].data_ptr())
    a.B, a.Hs, a.Ws, a.y0, a.x0, a.h, a.w = B, Hs, Ws, y0, x0, h, w
    per = {"u16": 2.0, "u8": 1.0, "rgb": 3.0, "err": 3.0}
    work = B * h * w * (4.0 + (4.0 if "err" in names else 0.0) + (1.0 if m is not None else 0.0) +
                        sum(per[n] for n in names) + ((4.0 + (1.0 if m is not None else 0.0)) if ws is not None else 0.0))
    with torch.cuda.device(dev), _timed("encode_range+rows" if ws is not None else "encode_rows", work):
        rc = lib.dsm_disp_encode(ctypes.byref(a), _stream())
    _lib.check(rc, "dsm_disp_encode")
    return out
