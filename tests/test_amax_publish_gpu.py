"""The tensor-maximum slot contract (csrc/split_core.hpp), once per publisher form, with a
caller-owned slot handed straight to the C entry points:

  4-wave    ``publish_amax<4>``: a plan-kind-5 split convolution, 2-D 64 -> 64 at 5 x 33 (ragged tiles in y and x);
  8-wave    ``publish_amax<8>``: the z-sliding convolution, 32 -> 32 at 2 x 9 x 33 (ragged tiles in y and x);
  per-wave  ``publish_amax_per_wave``: ``bn_apply`` at C = 32, 3 x 5 x 9 -- 1080 quads, a ragged last block.

a) a zeroed slot holds exactly max |y| after the launch; b) a slot that already holds 2 max |y| is left alone, bit
for bit; c) the maximum planted in the last element of y (in the ragged last tile / block) or in the first is
found; d) a null slot launches and returns DSM_OK.  Every f16x2 consumer reads these slots unchecked: they decide
whether fp16 overflows.

Second group: the producers no other test pins to the exact value, ``dy_amax`` and ``dres_amax`` of
``dsm_bn3d_train_bwd``, with a residual box one voxel larger than y in each extent (the cropped index path)."""
import ctypes

import pytest
import torch

from tests.helpers import seeded

pytestmark = pytest.mark.gpu
CL3D = torch.channels_last_3d
PLANTED = 1000.0                    # far above anything the seeded inputs produce


@pytest.fixture(scope="module")
def cv(hip_lib):
    from dsmnet_amd import costvolume
    return costvolume


def bits(t):
    return t.view(torch.int32).item()


def residual_with(shape, fmt, plant):
    """Skip tensor that plants the maximum of y: zeros but for PLANTED in the last / first element in memory."""
    if plant is None:
        return None
    r = torch.zeros(shape, device="cuda").contiguous(memory_format=fmt)
    idx = tuple(n - 1 for n in shape) if plant == "last" else (0,) * len(shape)
    r[idx] = PLANTED
    return r


# ------------------------------------------------------------------------------------ the three forms --
_DATA = {}


def conv_inputs(cv, form):
    """x, packed weights and x_amax of a convolution form, made once."""
    if form not in _DATA:
        if form == "4-wave":
            x = seeded(301, 1, 64, 5, 33).cuda().contiguous(memory_format=torch.channels_last)
            w = cv.pack_conv2d_weight(seeded(302, 64, 64, 3, 3, scale=(2.0 / (9 * 64)) ** 0.5).cuda())
        else:
            x = seeded(303, 1, 32, 2, 9, 33).cuda().contiguous(memory_format=CL3D)
            w = cv.pack_conv3d_weight(seeded(304, 32, 32, 3, 3, 3, scale=(2.0 / (27 * 32)) ** 0.5).cuda(), False)
        _DATA[form] = (x, w, cv.absmax(x))
    return _DATA[form]


def launch_conv(cv, form, slot, plant):
    """``dsm_conv3d_fwd`` in f16x2 with ``slot`` (or None) as y_amax -> (return code, y, plan name)."""
    from dsmnet_amd import _lib
    x, w, xa = conv_inputs(cv, form)
    two_d = form == "4-wave"
    fmt = torch.channels_last if two_d else CL3D
    y = torch.empty(tuple(x.shape), device="cuda").contiguous(memory_format=fmt)
    res = residual_with(tuple(x.shape), fmt, plant)
    a = _lib.Conv3dArgs()
    a.x, a.w_packed, a.y = x.data_ptr(), w.data_ptr(), y.data_ptr()
    a.residual = None if res is None else res.data_ptr()
    a.B, a.Cin, a.Cout = x.shape[0], x.shape[1], x.shape[1]
    a.Di, a.Hi, a.Wi = (1, x.shape[2], x.shape[3]) if two_d else tuple(x.shape[2:])
    a.Do, a.Ho, a.Wo = a.Dr, a.Hr, a.Wr = a.Di, a.Hi, a.Wi
    a.stride, a.relu, a.kd, a.k, a.dil = 1, 0, (1 if two_d else 3), 3, 1
    a.precision, a.x_amax = _lib.DSM_PREC_F16X2, xa.data_ptr()
    a.y_amax = None if slot is None else slot.data_ptr()
    name = cv.conv3d_plan_name(a)
    nws = _lib.load().dsm_conv3d_workspace_bytes(ctypes.byref(a))
    ws = torch.empty(max(nws // 4, 4), device="cuda")
    a.workspace, a.workspace_bytes = ws.data_ptr(), nws
    rc = _lib.load().dsm_conv3d_fwd(ctypes.byref(a), cv._stream())
    torch.cuda.synchronize()
    return rc, y, name


def bn_args(y, res_shape):
    from dsmnet_amd import _lib
    B, C, D, H, W = y.shape
    a = _lib.Bn3dArgs()
    a.B, a.C, a.Dy, a.Hy, a.Wy = B, C, D, H, W
    if res_shape is not None:
        a.Dr, a.Hr, a.Wr = res_shape[2:]
    keep = (torch.empty(4 * C, device="cuda"), torch.empty(2 * C, device="cuda", dtype=torch.float64))
    a.y, a.affine, a.workspace = y.data_ptr(), keep[0].data_ptr(), keep[1].data_ptr()
    a.relu, a.momentum, a.eps = 0, 0.1, 1e-5
    return a, keep


def launch_bn(cv, slot, plant):
    """``dsm_bn3d_train_fwd`` with ``slot`` (or None) as out_amax -> (return code, out, None)."""
    from dsmnet_amd import _lib
    if "bn" not in _DATA:
        _DATA["bn"] = seeded(305, 1, 32, 3, 5, 9).cuda().contiguous(memory_format=CL3D)
    y = _DATA["bn"]
    res = residual_with(tuple(y.shape), CL3D, plant)
    a, keep = bn_args(y, None if res is None else tuple(res.shape))
    out = torch.empty(tuple(y.shape), device="cuda").contiguous(memory_format=CL3D)
    a.out = out.data_ptr()
    a.residual = None if res is None else res.data_ptr()
    a.out_amax = None if slot is None else slot.data_ptr()
    rc = _lib.load().dsm_bn3d_train_fwd(ctypes.byref(a), cv._stream())
    torch.cuda.synchronize()
    return rc, out, None


FORMS = {"4-wave": "conv2d_f16x2_mfma_kernel<NT=2,TM=1,DIL=1>", "8-wave": "conv3d_zs_f16x2_mfma_kernel", "per-wave": None}


def launch(cv, form, slot, plant=None):
    rc, y, name = launch_bn(cv, slot, plant) if form == "per-wave" else launch_conv(cv, form, slot, plant)
    assert name == FORMS[form]                 # the kernel this case is meant for
    return rc, y


@pytest.mark.parametrize("form", list(FORMS))
def test_zeroed_slot_then_larger_slot_then_null_slot(cv, form):
    from dsmnet_amd import _lib
    slot = torch.zeros(1, device="cuda")
    rc, y = launch(cv, form, slot)
    want = y.abs().max().item()
    assert rc == _lib.DSM_OK and want > 0.0
    assert slot.item() == want                                   # a: exactly max |y|
    big = torch.full((1,), 2.0 * want, device="cuda")
    before = bits(big)
    rc, y2 = launch(cv, form, big)
    assert rc == _lib.DSM_OK and bits(big) == before             # b: left alone, bit for bit
    rc, y3 = launch(cv, form, None)
    assert rc == _lib.DSM_OK                                     # d: a null slot launches
    assert torch.equal(y2, y) and torch.equal(y3, y)


@pytest.mark.parametrize("plant", ["last", "first"])
@pytest.mark.parametrize("form", list(FORMS))
def test_maximum_planted_at_either_end(cv, form, plant):
    from dsmnet_amd import _lib
    slot = torch.zeros(1, device="cuda")
    rc, y = launch(cv, form, slot, plant)
    assert rc == _lib.DSM_OK
    flat = y.permute(0, *range(2, y.dim()), 1).reshape(-1)       # memory order: channels innermost
    at = flat.abs().argmax().item()
    assert at == (flat.numel() - 1 if plant == "last" else 0)    # c: the planted element IS the maximum
    assert slot.item() == flat.abs().max().item() and slot.item() > 0.5 * PLANTED


# --------------------------------------------------------------- producers without an exact assertion --
@pytest.mark.parametrize("relu", [1, 2])
def test_bn_backward_publishes_the_maxima_of_both_gradients(cv, relu):
    """``dy_amax`` / ``dres_amax`` of ``dsm_bn3d_train_bwd``: the residual box is one voxel larger than y in each
    extent, so dres is zero outside the common corner and every tensor takes the cropped index path."""
    from dsmnet_amd import _lib
    B, C, D, H, W = 1, 32, 3, 5, 9
    rshape = (B, C, D + 1, H + 1, W + 1)
    y = seeded(311, B, C, D, H, W).cuda().contiguous(memory_format=CL3D)
    res = seeded(312, *rshape).cuda().contiguous(memory_format=CL3D)
    gout = seeded(313, B, C, D, H, W).cuda().contiguous(memory_format=CL3D)
    gamma, beta = (seeded(314, C).abs() + 0.5).cuda(), seeded(315, C).cuda()
    out = torch.empty((B, C, D, H, W), device="cuda").contiguous(memory_format=CL3D)
    a, keep = bn_args(y, rshape)
    a.relu, a.gamma, a.beta = relu, gamma.data_ptr(), beta.data_ptr()
    a.residual, a.out = res.data_ptr(), out.data_ptr()
    _lib.check(_lib.load().dsm_bn3d_train_fwd(ctypes.byref(a), cv._stream()), "dsm_bn3d_train_fwd")
    dy = torch.empty_like(y, memory_format=CL3D)
    dres = torch.full(rshape, float("nan"), device="cuda").contiguous(memory_format=CL3D)
    slots = torch.zeros(8, device="cuda")                        # 16 bytes apart: two slots of one buffer
    a.residual = None
    a.gout, a.dy, a.dresidual = gout.data_ptr(), dy.data_ptr(), dres.data_ptr()
    a.dy_amax, a.dres_amax = slots[0:1].data_ptr(), slots[4:5].data_ptr()
    _lib.check(_lib.load().dsm_bn3d_train_bwd(ctypes.byref(a), cv._stream()), "dsm_bn3d_train_bwd")
    torch.cuda.synchronize()
    outside = dres.clone()
    outside[:, :, :D, :H, :W] = 0.0
    assert torch.isfinite(dres).all() and outside.abs().max().item() == 0.0             # written everywhere, zero outside
    assert dy.abs().max().item() > 0.0 and dres.abs().max().item() > 0.0
    assert slots[0].item() == dy.abs().max().item()
    assert slots[4].item() == dres.abs().max().item()
    assert slots[1:4].abs().max().item() == 0.0 and slots[5:].abs().max().item() == 0.0  # and nothing beside them
