"""GPU parity of the z-sliding transposed convolution (dsmnet_amd/csrc/deconv_zs.hpp; plan kind 6 in the
fp16 modes): ConvTranspose3d(k3, s2, p1, op1) with folded BN, optional cropped skip and ReLU -- conv5 and
conv6 of PSMNet's hourglass (models/psmnet/stackhourglass.py:35-49) -- against torch's float64 transposed
convolution on the CPU; results independent of how the work is cut into ranges; the output maximum."""
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import seeded
from tests.test_f16_gpu import F16X2_MAX, F16X2_RMS, F16_MAX, F16_RMS, errors, plan_of, precision
from tests.test_zs_gpu import with_grid

pytestmark = pytest.mark.gpu
LIMITS = {"f16x2": (F16X2_MAX, F16X2_RMS), "f16": (F16_MAX, F16_RMS)}


@pytest.fixture(scope="module")
def cv(hip_lib):
    from dsmnet_amd import costvolume
    return costvolume


def _reference(x, w, scale, shift, res, relu):
    y = F.conv_transpose3d(x.double(), w.double(), stride=2, padding=1, output_padding=1)
    y = y * scale.double().view(1, -1, 1, 1, 1) + shift.double().view(1, -1, 1, 1, 1)
    if relu == 2:
        y = y.relu()
    if res is not None:
        d, h, w_ = (min(a, b) for a, b in zip(y.shape[2:], res.shape[2:]))
        y = y[:, :, :d, :h, :w_] + res.double()[:, :, :d, :h, :w_]
    if relu == 1:
        y = y.relu()
    return y


def _inputs(B, cin, cout, dims, skip):
    x = seeded(41, B, cin, *dims)
    w = seeded(42, cin, cout, 3, 3, 3, scale=(2.0 / (27 * cout)) ** 0.5)
    scale, shift = seeded(43, cout).abs() + 0.5, seeded(44, cout)
    osz = tuple(2 * v for v in dims)
    res = None
    if skip == "full":
        res = seeded(45, B, cout, *osz)
    elif skip == "crop":
        res = seeded(45, B, cout, *(max(1, v - 1) for v in osz))
    return x, w, scale, shift, res


def _run(cv, mode, x, w, cout, scale, shift, res, relu, grid=0):
    old = with_grid(cv, grid)
    try:
        with precision(cv, mode):
            return cv.conv3d_block(x.cuda(), cv.pack_conv3d_weight(w.cuda(), True), cout, scale.cuda(), shift.cuda(),
                                   None if res is None else res.cuda(), 2, True, relu)
    finally:
        cv.set_option("conv_flags", old)


@pytest.mark.parametrize("B,dims,skip,relu,grid", [
    (1, (6, 12, 40), None, 0, 0),
    (2, (5, 7, 37), "full", 1, 0),          # batch 2, ragged in every dimension, odd Di
    (1, (1, 4, 32), None, 1, 0),            # one input plane: the second is the virtual plane
    (1, (3, 9, 70), "crop", 1, 7),          # skip shorter by one: odd output depth, ranges mid-column
    (2, (4, 6, 33), "full", 2, 5),          # GCNet: ReLU before the skip add
    (1, (1, 1, 1), "crop", 0, 0),           # smaller than a tile everywhere, cropped to 1 x 1 x 1
])
@pytest.mark.parametrize("cin,cout", [(64, 32), (64, 64)])
@pytest.mark.parametrize("mode", ["f16x2", "f16"])
def test_deconv_zs_vs_cpu_fp64(cv, mode, cin, cout, B, dims, skip, relu, grid):
    x, w, scale, shift, res = _inputs(B, cin, cout, dims, skip)
    with precision(cv, mode):
        assert "deconv3d_zs_%s_mfma" % mode in plan_of(cv, x, cout, 2, True, mode=mode)
    want = _reference(x, w, scale, shift, res, relu)
    y = _run(cv, mode, x, w, cout, scale, shift, res, relu, grid)
    assert tuple(y.shape) == tuple(want.shape)
    emax, erms = errors(y, want)
    assert emax <= LIMITS[mode][0] and erms <= LIMITS[mode][1], (emax, erms)
    assert y._dsm_amax.item() == y.abs().max().item()


@pytest.mark.parametrize("cin,cout,dims", [(64, 32, (7, 10, 45)), (64, 64, (5, 6, 70)), (128, 64, (3, 5, 33))])
@pytest.mark.parametrize("grid", [1, 3, 13, 61, 255])
def test_deconv_zs_ranges_do_not_change_the_bits(cv, cin, cout, dims, grid):
    """Forced grid sizes put range borders mid-column (a range then starts on an odd plane whose z-tap 2
    belongs to the previous range): every output voxel still sums the same terms in the same order."""
    x, w, scale, shift, res = _inputs(1, cin, cout, dims, "crop")
    base = _run(cv, "f16x2", x, w, cout, scale, shift, res, 1)
    y = _run(cv, "f16x2", x, w, cout, scale, shift, res, 1, grid)
    assert torch.equal(y, base)
    assert y._dsm_amax.item() == base._dsm_amax.item() == y.abs().max().item()


@pytest.mark.parametrize("mode", ["f16x2", "f16"])
def test_psmnet_transposed_layers_take_the_z_sliding_kernel(cv, mode):
    with precision(cv, mode):
        conv5 = plan_of(cv, torch.empty(1, 64, 12, 24, 80), 64, 2, True, mode=mode)
        conv6 = plan_of(cv, torch.empty(1, 64, 24, 48, 160), 32, 2, True, mode=mode)
    assert conv5 == "deconv3d_zs_%s_mfma_kernel<NT=2>" % mode, conv5
    assert conv6 == "deconv3d_zs_%s_mfma_kernel<NT=1>" % mode, conv6


def test_bf16x3_transposed_layers_stay_on_the_split_kernel(cv):
    with precision(cv, "bf16x3"):
        name = plan_of(cv, torch.empty(1, 64, 24, 48, 160), 32, 2, True, mode="bf16x3")
    assert "bf16x3" in name and "_zs_" not in name, name


@pytest.mark.parametrize("mode", ["f16x2", "f16"])
@pytest.mark.parametrize("cin,cout,dims", [(128, 64, (12, 16, 32)), (64, 64, (24, 32, 64)), (64, 32, (48, 64, 128)),
                                           (32, 32, (48, 64, 128))])
def test_gcnet_transposed_layers_get_a_plan(cv, mode, cin, cout, dims):
    with precision(cv, mode):
        name = plan_of(cv, torch.empty(1, cin, *dims), cout, 2, True, mode=mode)
    assert "_%s_" % mode in name and "mfma" in name, name
    assert ("_zs_" in name) == (cin % 64 == 0), name
