"""CPU: dispatch of the 5x5 stride-2 2-D layers (Cout 128 / 256; dsmnet_amd/csrc/conv_wide2d.hpp with K = 5, plan
kind 10 of ``dsm_conv3d_fwd``).

``dsm_conv3d_plan`` is host-only and shares its selection code with ``dsm_conv3d_fwd``: pointers are fake
addresses (16: aligned), never dereferenced.  ``blocks2d.k5_ok`` must admit exactly what the plan admits; it is
called with a stand-in that looks like an fp32 CUDA tensor (shape, dtype, is_cuda)."""
import ctypes

import pytest
import torch
import torch.nn as nn

from dsmnet_amd import _lib
from tests.test_wide2d_plans import A16, PREC, FakeCudaMap, plan, precision

# (Cin, Cout) of DispNet's conv2 (also DispNetC's and iResNet's) and conv3a
LAYERS = [(64, 128), (128, 256)]
UNSUPPORTED, ARG = -2, -1


def k5_args(cin=64, cout=128, hw=(24, 40), mode="f16x2", k=5, stride=2, dil=1, B=1, flags=0):
    a = _lib.Conv3dArgs()
    a.x = a.w_packed = a.y = a.x_amax = A16
    a.B, a.Cin, a.Cout = B, cin, cout
    a.Di, a.Hi, a.Wi = 1, hw[0], hw[1]
    a.Do, a.Ho, a.Wo = 1, (hw[0] - 1) // stride + 1, (hw[1] - 1) // stride + 1
    a.stride, a.transposed, a.relu = stride, 0, 1
    a.kd, a.k, a.dil = 1, k, dil
    a.precision, fl = PREC[mode]
    a.flags = fl | flags
    return a


def fields(name):
    return tuple(int(name.split(key)[1].split(",")[0].rstrip(">")) for key in ("N=", "KS=", "units="))


@pytest.mark.parametrize("mode", ["f16x2", "f16"])
@pytest.mark.parametrize("cin,cout", LAYERS)
def test_plan_names_the_k5_kernel(hip_lib, cin, cout, mode):
    rc, name = plan(hip_lib, k5_args(cin, cout, mode=mode))
    assert rc == 0 and name.startswith("conv2d_k5_%s_mfma_kernel<S=2,N=" % mode), (rc, name)
    assert not name.startswith("conv2d_wide_")
    n, ks, units = fields(name)
    assert n in (32, 64) and 1 <= ks <= cin // 16 and units % ((cout // n) * ks) == 0, name


def _residual(a):
    a.residual, a.Dr, a.Hr, a.Wr = A16, 1, a.Ho, a.Wo


def _crop(a):
    a.Ho -= 1


def _no_amax(a):
    a.x_amax = None


# (what, argument overrides, edit of the struct, code with k = 5,
#  what the SAME arguments give with k = 3 from 64 -> 128 and from 128 -> 256: unchanged by the 5x5 kind)
REFUSALS = [
    ("stride 1", dict(stride=1), None, UNSUPPORTED,
     (0, "conv2d_f16x2_mfma_kernel<NT=2,TM=2,DIL=1>x2"), (0, "conv2d_wide_f16x2_mfma_kernel<S=1,N=32,KS=8,units=128>")),
    ("dilation 2", dict(dil=2), None, UNSUPPORTED, (UNSUPPORTED, ""), (UNSUPPORTED, "")),
    ("Cin % 16", dict(cin=24), None, UNSUPPORTED, (UNSUPPORTED, ""), (UNSUPPORTED, "")),
    ("Cout 64", dict(cout=64), None, UNSUPPORTED,
     (0, "conv2d_mfma_kernel<S=2,NT=2,TM=1,K=3,DIL=1>"), (0, "conv2d_mfma_kernel<S=2,NT=2,TM=1,K=3,DIL=1>")),
    ("Cout 512", dict(cout=512), None, UNSUPPORTED,
     (0, "conv2d_wide_f16x2_mfma_kernel<S=2,N=32,KS=4,units=128>"), (0, "conv2d_wide_f16x2_mfma_kernel<S=2,N=32,KS=8,units=256>")),
    ("a residual", {}, _residual, UNSUPPORTED, (UNSUPPORTED, ""), (UNSUPPORTED, "")),
    ("a cropped output", {}, _crop, UNSUPPORTED, (UNSUPPORTED, ""), (UNSUPPORTED, "")),
    ("bf16x3", dict(mode="bf16x3"), None, UNSUPPORTED, (UNSUPPORTED, ""), (UNSUPPORTED, "")),
    ("fp32 MFMA", dict(mode="fp32"), None, UNSUPPORTED, (UNSUPPORTED, ""), (UNSUPPORTED, "")),
    ("wider than eight boxes", dict(hw=(8, 1186)), None, UNSUPPORTED,
     (UNSUPPORTED, ""), (0, "conv2d_wide_f16x2_mfma_kernel<S=2,N=64,KS=4,units=320>")),
    ("input past 2 GiB", dict(hw=(2048, 1024), B=4), None, UNSUPPORTED, (UNSUPPORTED, ""), (UNSUPPORTED, "")),
    ("no x_amax", {}, _no_amax, ARG, (UNSUPPORTED, ""), (ARG, "")),
]


@pytest.mark.parametrize("what,kw,edit,code,k3_128,k3_256", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_plan_refuses_what_the_kernel_does_not_cover(hip_lib, what, kw, edit, code, k3_128, k3_256):
    for (cin, cout), k3 in zip(LAYERS, (k3_128, k3_256)):
        base = dict(cin=cin, cout=cout)
        base.update(kw)
        a = k5_args(k=5, **base)
        if edit:
            edit(a)
        assert plan(hip_lib, a) == (code, ""), (what, cin, cout)
        if code == UNSUPPORTED:
            assert hip_lib.dsm_conv3d_workspace_bytes(ctypes.byref(a)) == 0
        a = k5_args(k=3, **base)
        if edit:
            edit(a)
        assert plan(hip_lib, a) == k3, (what, cin, cout)


def test_the_widest_map_the_geometry_holds(hip_lib):
    """Eight column blocks of 74 outputs: 5 rows of 2 x 76 slots fill the 768 of a staged box."""
    assert plan(hip_lib, k5_args(hw=(8, 1184)))[0] == 0          # Wo = 592
    assert plan(hip_lib, k5_args(hw=(8, 1185)))[0] == UNSUPPORTED  # Wo = 593
    assert plan(hip_lib, k5_args(hw=(1, 1)))[0] == 0


@pytest.mark.parametrize("cin,cout", [(16, 128), (64, 128), (128, 256), (48, 256)])
def test_packed_weight_bytes_are_the_fp16_section_alone(hip_lib, cin, cout):
    assert hip_lib.dsm_conv_packed_weight_bytes(cin, cout, 1, 5) == 16 + cin * cout * 25 * 4


def test_packed_weight_bytes_refuse_other_5x5_shapes(hip_lib):
    for cin, cout, kd in ((24, 128, 1), (64, 64, 1), (64, 512, 1), (64, 128, 3)):
        assert hip_lib.dsm_conv_packed_weight_bytes(cin, cout, kd, 5) == 0
    assert hip_lib.dsm_conv_packed_weight_bytes(64, 128, 1, 3) == 64 * 128 * 9 * (4 + 6 + 4) + 16     # as before


def test_both_model_rows_get_a_workgroup_per_cu(hip_lib):
    """conv2 and conv3a at 384 x 1280: units = M-blocks x N-columns x K-ranges >= 256, read back from the plan
    name, and the workspace size ([K][M][Cout] floats)."""
    for (cin, cout), hw in zip(LAYERS, ((192, 640), (96, 320))):
        for mode in ("f16x2", "f16"):
            a = k5_args(cin, cout, hw=hw, mode=mode)
            rc, name = plan(hip_lib, a)
            assert rc == 0, (cin, cout, mode)
            n, ks, units = fields(name)
            assert n in (32, 64) and 1 <= ks <= cin // 16
            assert units >= 256 and units % ((cout // n) * ks) == 0, name
            ws = hip_lib.dsm_conv3d_workspace_bytes(ctypes.byref(a))
            assert ws == (4 * ks * a.Ho * a.Wo * cout if ks > 1 else 0)


def test_forced_split_counts_are_clamped_as_for_the_wide_layers(hip_lib):
    """flags bits 8..13: at most one range per 16-channel chunk (and at least one per eight chunks)."""
    for cin, cout, forced, want in ((64, 128, 1, 1), (64, 128, 2, 2), (64, 128, 63, 4), (128, 256, 5, 5),
                                    (128, 256, 63, 8), (48, 256, 7, 3), (16, 128, 5, 1)):
        a = k5_args(cin, cout, flags=forced << _lib.DSM_CONV_KSPLIT_SHIFT)
        rc, name = plan(hip_lib, a)
        assert rc == 0 and ("KS=%d," % want) in name, (cin, forced, name)
        ws = hip_lib.dsm_conv3d_workspace_bytes(ctypes.byref(a))
        assert ws == (4 * want * a.Ho * a.Wo * cout if want > 1 else 0)


# (Cin of the map, conv (Cin, Cout, k, stride, padding, dilation), (B, H, W))
OK_CASES = [
    (64, (64, 128, 5, 2, 2, 1), (1, 192, 640)), (128, (128, 256, 5, 2, 2, 1), (1, 96, 320)),     # the model layers
    (64, (64, 128, 5, 2, 2, 1), (1, 24, 40)), (128, (128, 256, 5, 2, 2, 1), (2, 3, 5)),
    (64, (64, 128, 5, 1, 2, 1), (1, 24, 40)),            # stride 1
    (64, (64, 128, 5, 2, 4, 2), (1, 24, 40)),            # dilation 2
    (105, (105, 256, 5, 2, 2, 1), (1, 24, 40)),          # DispNetC's conv3a: Cin % 16
    (64, (64, 64, 5, 2, 2, 1), (1, 24, 40)),             # Cout
    (64, (64, 512, 5, 2, 2, 1), (1, 24, 40)),
    (64, (64, 128, 5, 2, 2, 1), (1, 8, 1186)),           # wider than eight boxes
    (64, (64, 128, 5, 2, 2, 1), (4, 2048, 1024)),        # input past 2 GiB
]


@pytest.mark.parametrize("mode", ["f16x2", "f16", "bf16x3", "fp32"])
def test_k5_ok_agrees_with_the_plan_and_fused_ok_stays_false(hip_lib, mode):
    from dsmnet_amd import blocks2d
    with precision(mode):
        for cin, (ci, co, k, s, p, d), (B, H, W) in OK_CASES:
            conv = nn.Conv2d(ci, co, k, s, padding=p, dilation=d)
            x = FakeCudaMap(B, cin, H, W)
            rc = plan(hip_lib, k5_args(ci, co, hw=(H, W), mode=mode, stride=s, dil=d, B=B))[0]
            assert blocks2d.k5_ok(conv, x) == (rc == 0), (mode, ci, co, s, d, (B, H, W), rc)
            assert blocks2d.fused_ok(conv, x) is False
        assert (plan(hip_lib, k5_args(64, 128, hw=(192, 640), mode=mode))[0] == 0) == (mode in ("f16x2", "f16"))


def test_k5_ok_refuses_what_is_no_such_layer(hip_lib):
    from dsmnet_amd import blocks2d
    x = FakeCudaMap(1, 64, 24, 40)
    assert blocks2d.k5_ok(nn.Conv2d(64, 128, 5, 2, padding=2), x)
    assert not blocks2d.k5_ok(nn.Conv2d(64, 128, 5, 2, padding=1), x)                    # not "same"
    assert not blocks2d.k5_ok(nn.Conv2d(64, 128, 5, 2, padding=2, groups=2), x)
    assert not blocks2d.k5_ok(nn.Conv2d(64, 128, 5, 2, padding=2, padding_mode="reflect"), x)
    assert not blocks2d.k5_ok(nn.Conv2d(64, 128, 3, 2, padding=1), x)
    assert not blocks2d.k5_ok(nn.Conv2d(64, 128, (5, 3), 2, padding=(2, 1)), x)
    assert not blocks2d.k5_ok(nn.Conv2d(48, 128, 5, 2, padding=2), x)                    # the map has other channels
    assert not blocks2d.k5_ok(nn.Conv2d(64, 128, 5, 2, padding=2), torch.zeros(1, 64, 24, 40))   # a CPU tensor
    assert not blocks2d.k5_ok(nn.ConvTranspose2d(64, 128, 5, 2, padding=2), x)


def test_split_kernel_layer_is_true_for_the_k5_launches():
    """These launches read ``x_amax``: the host must hand it over."""
    from dsmnet_amd import costvolume as cv
    for cin, cout in LAYERS + [(48, 256), (16, 128)]:
        assert cv._split_kernel_layer(k5_args(cin, cout)) is True
    assert cv._split_kernel_layer(k5_args(64, 128, stride=1)) is False
    assert cv._split_kernel_layer(k5_args(64, 128, dil=2)) is False
    assert cv._split_kernel_layer(k5_args(24, 128)) is False
    assert cv._split_kernel_layer(k5_args(64, 64)) is False


def test_the_option_is_off_by_default_and_switches():
    import os
    from dsmnet_amd import costvolume as cv
    if os.environ.get("DSM_CONV2D_K5", "") == "":
        assert cv.get_option("conv2d_k5") is False
    old = cv.set_option("conv2d_k5", 1)
    try:
        assert cv.get_option("conv2d_k5") is True
    finally:
        cv.set_option("conv2d_k5", old)
    assert "conv2d_k5" in cv.set_option.__doc__ and "DSM_CONV2D_K5" in cv.set_option.__doc__
