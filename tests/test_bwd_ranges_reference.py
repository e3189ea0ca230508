"""CPU: the float64 references of tests/test_bwd_ranges_gpu.py are accurate enough for its bounds.

A bound of 1e-4 (1e-5 for the heads' dx) against float64 autograd only judges the kernel if ordinary fp32
arithmetic on the same inputs lies well inside it.  For every shape the GPU tests list, torch's own fp32
CPU autograd must stay below a QUARTER of the tightest bound that applies to the shape; a shape that does
not would need a bound of its own (4 x its fp32 CPU error) in the GPU test.  Runs without a GPU, so a
shape added to those lists is checked when it is added."""
import pytest
import torch
import torch.nn.functional as F

from tests import test_bwd_ranges_gpu as T

LAYER_TOL = min(T.TOL.values())


def _rel(got, ref):
    return (got.detach().double() - ref).abs().max().item() / ref.abs().max().item()


def _assert_quarter(tag, ex, ew, tol_x, tol_w):
    print("%s: fp32 CPU autograd vs float64  dX %.2e  dW %.2e" % (tag, ex, ew))
    assert ex <= tol_x / 4, "%s: dX %.3e > %.1e / 4" % (tag, ex, tol_x)
    assert ew <= tol_w / 4, "%s: dW %.3e > %.1e / 4" % (tag, ew, tol_w)


@pytest.mark.parametrize("layer,shape", [(l, v) for l in T.LAYERS3D for v in T.VOLUMES] + T.BIG3D, ids=T._id)
def test_fp32_autograd_is_within_a_quarter_of_the_3d_bound(layer, shape):
    cin, cout, stride, transposed = layer
    x, w, cot, gx, gw = T.conv3d_case(layer, shape)
    xf, wf = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    if transposed:
        y = F.conv_transpose3d(xf, wf, None, stride=2, padding=1, output_padding=1)
    else:
        y = F.conv3d(xf, wf, None, stride=stride, padding=1)
    dx, dw = torch.autograd.grad(y, [xf, wf], cot)
    _assert_quarter("conv3d %s %s" % (T._id(layer), T._id(shape)), _rel(dx, gx), _rel(dw, gw), LAYER_TOL, LAYER_TOL)


@pytest.mark.parametrize("layer,shape", [(l, v) for l in T.LAYERS2D for v in T.MAPS] + T.BIG2D, ids=T._id)
def test_fp32_autograd_is_within_a_quarter_of_the_2d_bound(layer, shape):
    cin, cout, stride, dil = layer
    x, w, cot, gx, gw = T.conv2d_case(layer, shape)
    xf, wf = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(xf, wf, None, stride=stride, padding=dil, dilation=dil)
    dx, dw = torch.autograd.grad(y, [xf, wf], cot)
    _assert_quarter("conv2d %s %s" % (T._id(layer), T._id(shape)), _rel(dx, gx), _rel(dw, gw), LAYER_TOL, LAYER_TOL)


@pytest.mark.parametrize("C,shape", T.CONV_HEADS, ids=T._id)
def test_fp32_autograd_is_within_a_quarter_of_the_conv_head_bounds(C, shape):
    xn, w, g, gx, gw = T.conv_head_case(C, shape)
    xf, wf = xn.permute(0, 4, 1, 2, 3).clone().requires_grad_(True), w.clone().requires_grad_(True)
    dx, dw = torch.autograd.grad(F.conv3d(xf, wf, None, padding=1), [xf, wf], g.unsqueeze(1))
    _assert_quarter("conv head C=%d %s" % (C, T._id(shape)), _rel(dx.permute(0, 2, 3, 4, 1), gx), _rel(dw, gw),
                    T.HEAD_DX_TOL, T.HEAD_DW_TOL)


@pytest.mark.parametrize("crop", [0, 1])
@pytest.mark.parametrize("C,shape", T.DECONV_HEADS, ids=T._id)
def test_fp32_autograd_is_within_a_quarter_of_the_deconv_head_bounds(C, shape, crop):
    xn, w, g, gx, gw = T.deconv_head_case(C, shape, crop)
    xf, wf = xn.permute(0, 4, 1, 2, 3).clone().requires_grad_(True), w.clone().requires_grad_(True)
    Do, Ho, Wo = g.shape[1:]
    y = F.conv_transpose3d(xf, wf, None, stride=2, padding=1, output_padding=1)[:, :, :Do, :Ho, :Wo]
    dx, dw = torch.autograd.grad(y, [xf, wf], g.unsqueeze(1))
    _assert_quarter("deconv head C=%d %s crop %d" % (C, T._id(shape), crop), _rel(dx.permute(0, 2, 3, 4, 1), gx),
                    _rel(dw, gw), T.HEAD_DX_TOL, T.HEAD_DW_TOL)
