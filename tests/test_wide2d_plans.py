"""CPU: dispatch of the wide 3x3 2-D layers (256 / 512 / 1024 outputs; dsmnet_amd/csrc/conv_wide2d.hpp).

``dsm_conv3d_plan`` is host-only and shares its selection code with ``dsm_conv3d_fwd``: pointers are fake
addresses (16: aligned), never dereferenced.  ``blocks2d.fused_ok`` must admit exactly what the plan
admits; it is called with a stand-in that looks like an fp32 CUDA tensor (shape, dtype, is_cuda)."""
import ctypes
from contextlib import contextmanager

import pytest
import torch
import torch.nn as nn

from dsmnet_amd import _lib
from tests.helpers import golden_state

A16 = 16
PREC = {"f16x2": (_lib.DSM_PREC_F16X2, 0), "f16": (_lib.DSM_PREC_F16, 0),
        "bf16x3": (_lib.DSM_PREC_F32, 0), "fp32": (_lib.DSM_PREC_F32, _lib.DSM_CONV_FP32_MFMA)}
# (Cin, Cout, stride) of the encoder chain: conv3b, conv4a, conv4b / conv5a / conv5b, conv6a, conv6b
CHAIN = [(256, 256, 1), (256, 512, 2), (512, 512, 1), (512, 1024, 2), (1024, 1024, 1)]


def wide_args(cin, cout, stride, mode, hw=(12, 40), dil=1, B=1, flags=0):
    a = _lib.Conv3dArgs()
    a.x = a.w_packed = a.y = a.x_amax = A16
    a.B, a.Cin, a.Cout = B, cin, cout
    a.Di, a.Hi, a.Wi = 1, hw[0], hw[1]
    a.Do, a.Ho, a.Wo = 1, (hw[0] - 1) // stride + 1, (hw[1] - 1) // stride + 1
    a.stride, a.transposed, a.relu = stride, 0, 1
    a.kd, a.k, a.dil = 1, 3, dil
    a.precision, fl = PREC[mode]
    a.flags = fl | flags
    return a


def plan(hip_lib, a):
    buf = ctypes.create_string_buffer(96)
    rc = hip_lib.dsm_conv3d_plan(ctypes.byref(a), buf, 96)
    return rc, buf.value.decode()


class FakeCudaMap(object):
    """What ``fused_ok`` looks at: an fp32 CUDA tensor's type and shape, without a GPU."""
    is_cuda, dtype = True, torch.float32

    def __init__(self, *shape):
        self.shape = torch.Size(shape)


@contextmanager
def precision(mode):
    from dsmnet_amd import costvolume as cv
    old = cv.set_option("conv_precision", mode)
    try:
        yield
    finally:
        cv.set_option("conv_precision", old)


@pytest.mark.parametrize("mode", ["f16x2", "f16"])
@pytest.mark.parametrize("cin,cout,stride", CHAIN)
def test_plan_names_the_wide_kernel(hip_lib, cin, cout, stride, mode):
    rc, name = plan(hip_lib, wide_args(cin, cout, stride, mode))
    assert rc == 0 and name.startswith("conv2d_wide_%s_mfma_kernel<S=%d," % (mode, stride)), (rc, name)


@pytest.mark.parametrize("mode", ["bf16x3", "fp32"])
@pytest.mark.parametrize("cin,cout,stride", CHAIN)
def test_plan_refuses_the_wide_layers_outside_the_fp16_modes(hip_lib, cin, cout, stride, mode):
    assert plan(hip_lib, wide_args(cin, cout, stride, mode)) == (-2, "")


def test_plan_refuses_what_the_kernel_does_not_cover(hip_lib):
    assert plan(hip_lib, wide_args(256, 384, 1, "f16x2"))[0] == -2          # Cout
    assert plan(hip_lib, wide_args(24, 256, 1, "f16x2"))[0] == -2           # Cin % 16
    assert plan(hip_lib, wide_args(256, 256, 1, "f16x2", dil=2))[0] == -2   # dilation
    a = wide_args(256, 256, 1, "f16x2")
    a.residual, a.Dr, a.Hr, a.Wr = A16, 1, a.Ho, a.Wo
    assert plan(hip_lib, a)[0] == -2                                        # no skip input
    a = wide_args(256, 256, 1, "f16x2")
    a.x_amax = None
    assert plan(hip_lib, a)[0] == -1                                        # the input's maximum is required


def test_every_table_row_gets_a_workgroup_per_cu(hip_lib):
    """The seven layers at 384 x 1280: units = M-blocks x N-columns x K-ranges >= 256, read back from the
    plan name ("<S,N,KS,units>") and the workspace size ([K][M][Cout] floats)."""
    rows = [(256, 256, 1, (48, 160)), (256, 512, 2, (48, 160)), (512, 512, 1, (24, 80)), (512, 512, 2, (24, 80)),
            (512, 512, 1, (12, 40)), (512, 1024, 2, (12, 40)), (1024, 1024, 1, (6, 20))]
    for cin, cout, s, hw in rows:
        a = wide_args(cin, cout, s, "f16x2", hw=hw)
        rc, name = plan(hip_lib, a)
        assert rc == 0, (cin, cout, s)
        n, ks, units = (int(name.split(key)[1].split(",")[0].rstrip(">")) for key in ("N=", "KS=", "units="))
        assert n in (32, 64) and 1 <= ks <= cin // 16
        assert units >= 256 and units % ((cout // n) * ks) == 0, name       # M-blocks x N-columns x K-ranges
        ws = hip_lib.dsm_conv3d_workspace_bytes(ctypes.byref(a))
        assert ws == (4 * ks * a.Ho * a.Wo * cout if ks > 1 else 0)


def test_forced_split_counts_are_clamped_to_what_the_kernel_supports(hip_lib):
    """flags bits 8..13: at most one range per 16-channel chunk, at least one per eight chunks (a longer
    fp32 accumulation chain would leave the f16x2 error band)."""
    for cin, forced, want in ((1024, 1, 8), (1024, 16, 16), (1024, 63, 63), (256, 1, 2), (48, 7, 3), (16, 5, 1)):
        a = wide_args(cin, 256, 1, "f16x2", flags=forced << _lib.DSM_CONV_KSPLIT_SHIFT)
        rc, name = plan(hip_lib, a)
        assert rc == 0 and ("KS=%d," % want) in name, (cin, forced, name)


@pytest.mark.parametrize("mode", ["f16x2", "f16", "bf16x3", "fp32"])
def test_fused_ok_agrees_with_the_plan(hip_lib, mode):
    from dsmnet_amd import blocks2d
    cases = [(cin, cout, s, 3, 1) for cin, cout, s in CHAIN]
    cases += [(256, 384, 1, 3, 1), (24, 256, 1, 3, 1), (256, 256, 1, 3, 2), (105, 256, 2, 5, 1), (145, 256, 2, 3, 1),
              (1025, 512, 1, 3, 1)]
    with precision(mode):
        for cin, cout, s, k, dil in cases:
            conv = nn.Conv2d(cin, cout, k, s, padding=dil * (k - 1) // 2, dilation=dil)
            ok = blocks2d.fused_ok(conv, FakeCudaMap(1, cin, 12, 40))
            rc = -2 if k != 3 else plan(hip_lib, wide_args(cin, cout, s, mode, dil=dil))[0]
            assert ok == (rc == 0), (mode, cin, cout, s, k, dil, ok, rc)


def test_dispnetcorr_state_dict_keys_are_the_checkpoint_contract(golden_e2e):
    from dsmnet_amd.models import model_create_by_name
    from dsmnet_amd.models.util_conv import Conv2dReLU
    sd, _ = golden_state(golden_e2e, "dispnetcorr")
    m = model_create_by_name("dispnetcorr", 192)
    assert set(m.state_dict().keys()) == set(sd.keys())
    m.load_state_dict(sd, strict=True)
    assert isinstance(m.conv6b, Conv2dReLU) and isinstance(m.conv6b[0], nn.Conv2d) and isinstance(m.conv6b[1], nn.ReLU)
