"""GPU parity of the BACKWARD kernels (dsmnet_amd/csrc/conv3d_bwd.hip) where their workgroups carry
state from one work unit to the next.

The weight-gradient kernels are persistent: a workgroup walks a contiguous range of (column, z) units,
keeps its accumulators across them and (27-tap layers) re-stages only the X planes a step along z
brings in.  At the small shapes of the other gradient tests there are fewer units than workgroups,
every range is one unit long and none of that state is used.  Here the grid size is FORCED
(bits 16..31 of the wgrad ``flags``, ``conv_flags`` option) to 1, 2, 3, 7 workgroups per channel pair
-- one workgroup walking every column change, batch change and ring reuse; range borders in the
middle of a column and of a batch item -- next to the launcher's own choice (0), on batch-2 volumes
that are ragged in y and x; and a few shapes with more units than the default grid has workgroups.
The Cout = 1 head backward entry points (``dsm_conv3d_cout1_bwd``, ``dsm_deconv3d_cout1_bwd``) are
called directly: every kernel they dispatch to, ranges of several tiles, dx-only / dw-only calls.

Reference: float64 CPU autograd of F.conv3d / F.conv_transpose3d / F.conv2d on the same seeded
inputs.  Errors are relative to the largest entry of the reference gradient.

Bounds.  bf16x3, f16x2 and the exact fp32 kernel: 1e-4 (GRAD_TOL of tests/test_conv3d_bwd_gpu.py);
f16: 4e-3 (tests/test_train_f16_gpu.py).  Head kernels (plain fp32 FMA chains and atomics): dx 1e-5,
dw 1e-4.  These hold only where the float64 reference is not the limiting party: torch's own fp32 CPU
autograd on the same inputs stays far below a quarter of every bound at every shape listed here --
worst over all cases (measured with 16 host threads): 3-D layers dX 8.9e-7, dW 3.1e-6; 2-D layers
dX 5.2e-7, dW 2.7e-6; conv head dx 2.6e-7, dw 5.1e-7; transposed head dx 2.3e-7, dw 1.3e-6 -- so no
shape needs a bound of its own.  tests/test_bwd_ranges_reference.py keeps that checked, without a GPU,
for every case list of this file.
The results of one case at the different grids differ only by summation order and must agree with
each other to the same bound: a stale ring plane or a dropped unit is an O(1) relative difference."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import seeded

pytestmark = pytest.mark.gpu

GRIDS = (1, 2, 3, 7, 0)
MODES = ("bf16x3", "f16x2", "f16", "fp32")
TOL = {"bf16x3": 1e-4, "f16x2": 1e-4, "f16": 4e-3, "fp32": 1e-4}
HEAD_DX_TOL, HEAD_DW_TOL = 1e-5, 1e-4

# (cin, cout, stride, transposed)
LAYERS3D = [(32, 32, 1, False), (64, 32, 1, False), (64, 64, 1, False), (32, 64, 2, False),
            (64, 64, 2, False), (64, 32, 2, True), (64, 64, 2, True)]
VOLUMES = [(2, 5, 9, 37), (2, 7, 18, 70)]
# (cin, cout, stride, dilation)
# (dX of 32 -> 64 s2 and of 320 -> 128 comes from aten.convolution_backward -- Conv2dFunction has no kernel
# for them: for those two layers only dW exercises a kernel of this project)
LAYERS2D = [(32, 32, 1, 1), (64, 64, 1, 1), (128, 128, 1, 2), (32, 64, 2, 1), (320, 128, 1, 1)]
MAPS = [(2, 21, 45), (2, 40, 70)]
# more units than the DEFAULT grid has workgroups (min(256 / pairs, units)), one per kernel family:
#   3-D 32 -> 32 s1: 2 * 12 * 10 * 3 = 720 units over 256;  64 -> 64 s2 (4 pairs, 64 workgroups): dY is
#   (2, 6, 19, 35), 456 one-row units (240 two-row units on the fp32 kernel);  2-D 128 -> 128 (16 pairs,
#   16 workgroups): 2 * 8 * 4 = 64 tiles;  2-D 32 -> 32: 2 * 21 * 19 = 798 tiles over 256
BIG3D = [((32, 32, 1, False), (2, 12, 37, 70)), ((64, 64, 2, False), (2, 12, 37, 70))]
BIG2D = [((128, 128, 1, 1), (2, 61, 100)), ((32, 32, 1, 1), (2, 161, 600))]

_WORST = {}


@pytest.fixture(scope="module")
def cv(hip_lib):
    from dsmnet_amd import costvolume
    yield costvolume
    print()
    for key in sorted(_WORST):
        print("worst relative error vs float64, %-22s dX %.2e  dW %.2e" % ((key,) + tuple(_WORST[key])))


def _note(key, ex, ew):
    old = _WORST.get(key, (0.0, 0.0))
    _WORST[key] = (max(old[0], ex), max(old[1], ew))


def _rel(got, ref):
    return (got.detach().double().cpu() - ref).abs().max().item() / ref.abs().max().item()


def _where(got, ref):
    """Index and values of the worst entry: which tap / channel pair / batch item is off."""
    err = (got.detach().double().cpu() - ref).abs()
    idx = tuple(int(i) for i in torch.nonzero(err == err.max())[0])
    return "worst at %r: got %.6e, want %.6e" % (idx, got.detach().double().cpu()[idx].item(), ref[idx].item())


@functools.lru_cache(maxsize=1)
def conv3d_case(layer, shape):
    """Inputs and float64 gradients of one 3-D layer (also used by the CPU bound check)."""
    cin, cout, stride, transposed = layer
    B, D, H, W = shape
    x = seeded(1, B, cin, D, H, W)
    w = seeded(2, *((cin, cout, 3, 3, 3) if transposed else (cout, cin, 3, 3, 3)), scale=0.1)
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    if transposed:
        ref = F.conv_transpose3d(xd, wd, None, stride=2, padding=1, output_padding=1)
    else:
        ref = F.conv3d(xd, wd, None, stride=stride, padding=1)
    cot = seeded(4, *ref.shape)
    gx, gw = torch.autograd.grad(ref, [xd, wd], cot.double())
    return x, w, cot, gx, gw


@functools.lru_cache(maxsize=1)
def conv2d_case(layer, shape):
    cin, cout, stride, dil = layer
    B, H, W = shape
    x = seeded(1, B, cin, H, W)
    w = seeded(2, cout, cin, 3, 3, scale=0.1)
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    ref = F.conv2d(xd, wd, None, stride=stride, padding=dil, dilation=dil)
    cot = seeded(4, *ref.shape)
    gx, gw = torch.autograd.grad(ref, [xd, wd], cot.double())
    return x, w, cot, gx, gw


def _gradients_at_grids(cv, mode, grids, x, w, cot, run):
    """{grid: (dx, dw)} of ``run(xg, wg)`` with the persistent grid size forced."""
    from dsmnet_amd import _lib
    out = {}
    old_mode = cv.set_option("conv_precision", mode)
    old_flags = cv.get_option("conv_flags")
    try:
        for grid in grids:
            cv.set_option("conv_flags", grid << _lib.DSM_CONV_BLOCKS_SHIFT)
            xg, wg = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
            y = run(xg, wg)
            dx, dw = torch.autograd.grad(y, [xg, wg], cot.cuda())
            out[grid] = (dx.detach().double().cpu(), dw.detach().double().cpu())
    finally:
        cv.set_option("conv_flags", old_flags)
        cv.set_option("conv_precision", old_mode)
    return out


def _check(tag, mode, got, gx, gw):
    tol = TOL[mode]
    worst = (0.0, 0.0)
    for grid, (dx, dw) in got.items():
        assert dx.shape == gx.shape and dw.shape == gw.shape
        ex, ew = _rel(dx, gx), _rel(dw, gw)
        worst = (max(worst[0], ex), max(worst[1], ew))
        print("%s %s grid %d: dX %.2e dW %.2e (bound %.0e)" % (tag, mode, grid, ex, ew, tol))
    _note(tag.split()[0] + " " + mode, *worst)
    for grid, (dx, dw) in got.items():
        ex, ew = _rel(dx, gx), _rel(dw, gw)
        assert ew <= tol, "%s %s grid %d: dW %.3e > %.0e; %s" % (tag, mode, grid, ew, tol, _where(dw, gw))
        assert ex <= tol, "%s %s grid %d: dX %.3e > %.0e; %s" % (tag, mode, grid, ex, tol, _where(dx, gx))
    grids = list(got)
    for grid in grids[1:]:                              # summation order only
        for name, a, b, ref in (("dW", got[grid][1], got[grids[0]][1], gw), ("dX", got[grid][0], got[grids[0]][0], gx)):
            diff = (a - b).abs().max().item() / ref.abs().max().item()
            assert diff <= tol, "%s %s: %s at grid %d and at grid %d differ by %.3e" % (
                tag, mode, name, grid, grids[0], diff)


def _id(v):
    return "x".join(str(int(i)) for i in v) if isinstance(v, tuple) else str(v)


_CASES3D = [(l, v, m, GRIDS) for l in LAYERS3D for v in VOLUMES for m in MODES] + \
           [(l, v, m, (0,)) for l, v in BIG3D for m in MODES]
_CASES2D = [(l, v, m, GRIDS) for l in LAYERS2D for v in MAPS for m in MODES] + \
           [(l, v, m, (0,)) for l, v in BIG2D for m in MODES]


@pytest.mark.parametrize("layer,shape,mode,grids", _CASES3D, ids=_id)
def test_conv3d_gradients_over_forced_ranges(cv, layer, shape, mode, grids):
    """dX and dW of Conv3d(s1 | s2) / ConvTranspose3d(s2) at every forced grid size against float64."""
    cin, cout, stride, transposed = layer
    x, w, cot, gx, gw = conv3d_case(layer, shape)
    got = _gradients_at_grids(cv, mode, grids, x, w, cot,
                              lambda xg, wg: cv.conv3d(xg, wg, None, stride, transposed))
    _check("conv3d %s %s" % (_id(layer), _id(shape)), mode, got, gx, gw)


@pytest.mark.parametrize("layer,shape,mode,grids", _CASES2D, ids=_id)
def test_conv2d_gradients_over_forced_ranges(cv, layer, shape, mode, grids):
    """The same for the towers' 3x3 layers (nine taps: every wave owns all taps and a quarter of the
    tile, the four waves' sums are folded through LDS)."""
    cin, cout, stride, dil = layer
    x, w, cot, gx, gw = conv2d_case(layer, shape)
    got = _gradients_at_grids(cv, mode, grids, x, w, cot, lambda xg, wg: cv.conv2d(xg, wg, stride, dil))
    _check("conv2d %s %s" % (_id(layer), _id(shape)), mode, got, gx, gw)


# ---- Cout = 1 heads, called as Conv3dFunction.backward calls them ------------------------------
def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=1)
def conv_head_case(C, shape):
    """x as NDHWC memory, g (B,D,H,W), w (1,C,3,3,3); float64 dx (NDHWC) and dw."""
    B, D, H, W = shape
    xn = seeded(11, B, D, H, W, C)
    w = seeded(12, 1, C, 3, 3, 3, scale=0.1)
    g = seeded(13, B, D, H, W)
    xd = xn.double().permute(0, 4, 1, 2, 3).requires_grad_(True)
    wd = w.double().requires_grad_(True)
    y = F.conv3d(xd, wd, None, padding=1)
    gx, gw = torch.autograd.grad(y, [xd, wd], g.double().unsqueeze(1))
    return xn, w, g, gx.permute(0, 2, 3, 4, 1).contiguous(), gw


@functools.lru_cache(maxsize=1)
def deconv_head_case(C, shape, crop):
    """ConvTranspose3d(C -> 1, k3, s2, p1, op1), the output cropped to (Do,Ho,Wo) = 2 (Di,Hi,Wi) - crop."""
    B, Di, Hi, Wi = shape
    Do, Ho, Wo = 2 * Di - crop, 2 * Hi - crop, 2 * Wi - crop
    xn = seeded(21, B, Di, Hi, Wi, C)
    w = seeded(22, C, 1, 3, 3, 3, scale=0.1)
    g = seeded(23, B, Do, Ho, Wo)
    xd = xn.double().permute(0, 4, 1, 2, 3).requires_grad_(True)
    wd = w.double().requires_grad_(True)
    y = F.conv_transpose3d(xd, wd, None, stride=2, padding=1, output_padding=1)[:, :, :Do, :Ho, :Wo]
    gx, gw = torch.autograd.grad(y, [xd, wd], g.double().unsqueeze(1))
    return xn, w, g, gx.permute(0, 2, 3, 4, 1).contiguous(), gw


def _conv_head(lib, xn, packed, g, want_dx, want_dw):
    B, D, H, W, C = xn.shape
    dx = torch.empty_like(xn) if want_dx else None
    dwt = torch.empty(27 * C, device=xn.device, dtype=torch.float32) if want_dw else None
    rc = lib.dsm_conv3d_cout1_bwd(_ptr(xn), _ptr(g), _ptr(packed), _ptr(dx), _ptr(dwt), B, C, D, H, W, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    dw = None if dwt is None else dwt.view(27, C).t().contiguous().view(1, C, 3, 3, 3)
    return dx, dw


CONV_HEADS = [
    (32, (2, 9, 20, 70)),      # 1080 tiles over 256 workgroups: ~4 per range, crossing rows and planes (the
                               # batch border, tile 540 = 1080 * 128 / 256, is a range border: next case)
    (32, (3, 9, 20, 70)),      # 1620 tiles, batch borders at 540 and 1080: 256 is no multiple of 3, so ranges
                               # [537, 544) and [1075, 1082) step from one batch item into the next
    (32, (1, 3, 5, 31)),       # W below a tile's width
    (64, (2, 9, 20, 70)),      # the 16-voxel tile kernel (1800 tiles; batch border on a range border again)
    (64, (3, 9, 20, 70)),      # 2700 tiles, batch borders at 900 and 1800 inside ranges [896, 907), [1792, 1803)
    (64, (1, 3, 5, 15)),
    (16, (2, 5, 9, 37)),       # the generic kernels
    (48, (2, 5, 9, 37)),
]
DECONV_HEADS = [
    (32, (2, 7, 20, 70)),      # 19 600 voxels over 2048 workgroups x 8 slots: the grid-stride loop iterates
    (32, (2, 3, 5, 9)), (48, (2, 3, 5, 9)), (64, (2, 3, 5, 9)), (256, (2, 3, 5, 9)),
    (48, (2, 7, 20, 70)),      # 256 / 48 = 5 voxel slots (16 idle threads), the loop iterates
]


@pytest.mark.parametrize("C,shape", CONV_HEADS, ids=_id)
def test_conv_head_backward_entry_point(cv, hip_lib, C, shape):
    xn, w, g, gx, gw = conv_head_case(C, shape)
    xg, gg = xn.cuda(), g.cuda()
    packed = w[0].reshape(C, 27).t().contiguous().cuda()             # [tap][cin]
    if C == 32:
        assert torch.equal(cv.pack_conv3d_weight(w.cuda(), False)[:27 * C], packed.view(-1))
    dx, dw = _conv_head(hip_lib, xg, packed, gg, True, True)
    ex, ew = _rel(dx, gx), _rel(dw, gw)
    print("conv head C=%d %s: dx %.2e dw %.2e" % (C, _id(shape), ex, ew))
    _note("conv-head fp32", ex, ew)
    assert ex <= HEAD_DX_TOL, "dx %.3e; %s" % (ex, _where(dx, gx))
    assert ew <= HEAD_DW_TOL, "dw %.3e; %s" % (ew, _where(dw, gw))
    dx_only, none = _conv_head(hip_lib, xg, packed, gg, True, False)
    assert none is None and torch.equal(dx_only, dx)
    none, dw_only = _conv_head(hip_lib, xg, packed, gg, False, True)
    assert none is None and _rel(dw_only, gw) <= HEAD_DW_TOL, _where(dw_only, gw)


def _deconv_head(lib, xn, w, g, want_dx, want_dw):
    B, Di, Hi, Wi, C = xn.shape
    dx = torch.empty_like(xn) if want_dx else None
    dw = torch.empty_like(w) if want_dw else None
    rc = lib.dsm_deconv3d_cout1_bwd(_ptr(xn), _ptr(g), _ptr(w), _ptr(dx), _ptr(dw), B, C, Di, Hi, Wi,
                                    g.shape[1], g.shape[2], g.shape[3], _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return dx, dw


@pytest.mark.parametrize("crop", [0, 1])
@pytest.mark.parametrize("C,shape", DECONV_HEADS, ids=_id)
def test_deconv_head_backward_entry_point(hip_lib, C, shape, crop):
    xn, w, g, gx, gw = deconv_head_case(C, shape, crop)
    xg, wg, gg = xn.cuda(), w.cuda(), g.cuda()
    dx, dw = _deconv_head(hip_lib, xg, wg, gg, True, True)
    ex, ew = _rel(dx, gx), _rel(dw, gw)
    print("deconv head C=%d %s crop %d: dx %.2e dw %.2e" % (C, _id(shape), crop, ex, ew))
    _note("deconv-head fp32", ex, ew)
    assert ex <= HEAD_DX_TOL, "dx %.3e; %s" % (ex, _where(dx, gx))
    assert ew <= HEAD_DW_TOL, "dw %.3e; %s" % (ew, _where(dw, gw))
    dx_only, none = _deconv_head(hip_lib, xg, wg, gg, True, False)
    assert none is None and torch.equal(dx_only, dx)
    none, dw_only = _deconv_head(hip_lib, xg, wg, gg, False, True)
    assert none is None and _rel(dw_only, gw) <= HEAD_DW_TOL, _where(dw_only, gw)


def test_head_backward_rejects_unaligned_quad_operands(hip_lib):
    """Both bwd-data kernels of the conv head read w_packed and write dx as 16-byte quads, the transposed
    head writes dx as quads: an address that is not 16-byte aligned is refused (DSM_ERR_ALIGN) before
    anything is launched.  Real device buffers of sufficient size, the unaligned one a view one float in:
    should a check ever move behind a launch, this shows as a return code or an overwritten dw, on valid
    memory."""
    def buf(fill=0.0):
        return torch.full((1028,), fill, device="cuda", dtype=torch.float32)   # >= 27 * 32, 8 * 32, 4^3 floats

    x, g, w, dx, dw = buf(), buf(), buf(), buf(), buf(7.0)
    w_off, dx_off = w[1:], dx[1:]
    assert dx.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0 and dx_off.data_ptr() % 16 == 4
    s = _stream()
    f = hip_lib.dsm_conv3d_cout1_bwd
    for C in (32, 16):
        assert f(_ptr(x), _ptr(g), _ptr(w), _ptr(dx_off), None, 1, C, 2, 2, 2, s) == -4       # dx
        assert f(_ptr(x), _ptr(g), _ptr(w_off), _ptr(dx), None, 1, C, 2, 2, 2, s) == -4       # w_packed
        assert f(_ptr(x), _ptr(g), _ptr(w), _ptr(dx_off), _ptr(dw), 1, C, 2, 2, 2, s) == -4   # before the dw launch too
    assert f(_ptr(x), _ptr(g), None, _ptr(dx), None, 1, 32, 2, 2, 2, s) == -1                 # dx without weights
    assert f(None, _ptr(g), _ptr(w), None, _ptr(dw), 1, 32, 2, 2, 2, s) == -1                 # dw without x
    d = hip_lib.dsm_deconv3d_cout1_bwd
    assert d(_ptr(x), _ptr(g), _ptr(w), _ptr(dx_off), None, 1, 32, 2, 2, 2, 4, 4, 4, s) == -4
    assert d(_ptr(x), _ptr(g), _ptr(w), _ptr(dx_off), _ptr(dw), 1, 32, 2, 2, 2, 4, 4, 4, s) == -4
    assert d(None, _ptr(g), _ptr(w), None, _ptr(dw), 1, 32, 2, 2, 2, 4, 4, 4, s) == -1
    torch.cuda.synchronize()
    assert bool((dw == 7.0).all()) and bool((dx == 0.0).all())          # nothing ran: not even dw's memset
