"""GPU parity of the first convolution of a concatenation cost volume computed from 2-D maps
(dsmnet_amd/csrc/sepvol.hip, ``costvolume.concat_conv_block``) against torch's float64
convolution of the volume ``oracle.ops.concat_volume`` builds, in the band the z-sliding kernel it
replaces is held to (tests/test_zs_gpu.py: test_virtual_volume_equals_the_materialised_one); and of the
models that reach it through ``blocks3d.run_block`` (option ``separable_volume``)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from oracle import ops as OO
from tests.helpers import maxerr, seeded
from tests.test_f16_gpu import F16X2_MAX, F16X2_RMS, errors, precision

pytestmark = pytest.mark.gpu
DISP_TOL = 1e-3


@pytest.fixture(scope="module")
def cv(hip_lib):
    from dsmnet_amd import costvolume
    return costvolume


def option(cv, name, value):
    class _Ctx(object):
        def __enter__(self):
            self.old = cv.set_option(name, value)

        def __exit__(self, *exc):
            cv.set_option(name, self.old)
            return False
    return _Ctx()


SHAPES = [
    # (B, C, H, W), D, separable_flags
    ((2, 32, 11, 53), 14, 0), ((1, 32, 9, 33), 40, 0), ((1, 64, 5, 70), 6, 0),      # those of the z-sliding test (D > W included)
    ((1, 32, 6, 9), 1, 0), ((1, 32, 6, 9), 2, 0), ((1, 32, 6, 9), 3, 0),            # small D
    ((1, 32, 4, 1), 5, 0), ((1, 32, 4, 4), 5, 0), ((1, 32, 4, 5), 5, 0),            # small W
    ((2, 64, 3, 1), 1, 0),
    ((1, 32, 7, 41), 13, 3 | (16 << 8)),                                           # ragged workgroup tiles: 3 planes x 16 columns
    ((1, 32, 4, 320), 48, 0),                                                      # the benchmark's width and depth
]


@pytest.mark.parametrize("mask_left", [False, True])
@pytest.mark.parametrize("shape,D,flags", SHAPES)
def test_concat_conv_vs_cpu_fp64(cv, shape, D, flags, mask_left):
    B, C, H, W = shape
    fL, fR = seeded(41, *shape), seeded(42, *shape)
    w = seeded(43, 32, 2 * C, 3, 3, 3, scale=0.04)
    scale, shift = seeded(44, 32).abs() + 0.5, seeded(45, 32)
    vol = OO.concat_volume(fL, fR, D, mask_left=mask_left)
    want = F.conv3d(vol.double(), w.double(), padding=1)
    want = (want * scale.double().view(1, -1, 1, 1, 1) + shift.double().view(1, -1, 1, 1, 1)).relu()
    both = torch.cat([fL, fR], 0).cuda().contiguous(memory_format=torch.channels_last)
    sep = cv.pack_concat_conv_weight(w.cuda())
    # poison what the allocator is about to hand out: an element the kernels leave unwritten is a NaN
    junk = torch.full((B * 32 * D * H * W,), float("nan"), device="cuda")
    del junk
    with option(cv, "separable_flags", flags):
        y = cv.concat_conv_block(cv.VirtualVolume(both, D, mask_left), sep, scale.cuda(), shift.cuda(), relu=True)
    assert tuple(y.shape) == (B, 32, D, H, W) and y.is_contiguous(memory_format=torch.channels_last_3d)
    assert bool(torch.isfinite(y).all())
    emax, erms = errors(y, want)                 # every element
    grow = max(1.0, 2 * C / 64.0) ** 0.5
    print("concat_conv %s D=%d mask_left=%s: max %.3g rms %.3g" % (shape, D, mask_left, emax, erms))
    assert emax <= F16X2_MAX * grow and erms <= F16X2_RMS * grow, (emax, erms)
    assert y._dsm_amax.item() == y.abs().max().item()


def test_no_affine_no_relu_and_negative_values(cv):
    """scale / shift NULL, no ReLU: the absolute maximum is taken over negative values too."""
    shape, D = (1, 32, 5, 19), 7
    fL, fR = seeded(51, *shape), seeded(52, *shape)
    w = seeded(53, 32, 64, 3, 3, 3, scale=0.04)
    want = F.conv3d(OO.concat_volume(fL, fR, D, mask_left=True).double(), w.double(), padding=1)
    both = torch.cat([fL, fR], 0).cuda().contiguous(memory_format=torch.channels_last)
    y = cv.concat_conv_block(cv.VirtualVolume(both, D, True), cv.pack_concat_conv_weight(w.cuda()))
    emax, erms = errors(y, want)
    assert emax <= F16X2_MAX and erms <= F16X2_RMS, (emax, erms)
    assert y._dsm_amax.item() == y.abs().max().item()


def test_argument_validation_and_the_fallback(cv, hip_lib, monkeypatch):
    null, one = None, ctypes.c_void_p(16)

    def call(both=one, w=one, ws=one, nws=1 << 40, y=one, B=1, C=32, cout=32, D=4, H=4, W=8):
        return hip_lib.dsm_concat_conv_fwd(both, w, null, null, ws, nws, y, null, B, C, cout, D, H, W, 1, 1, 0, null)
    assert call(both=null) == -1 and call(w=null) == -1 and call(ws=null) == -1 and call(y=null) == -1
    assert call(C=48) == -1 and call(cout=64) == -1
    assert call(D=0) == -1 and call(H=0) == -1 and call(W=0) == -1
    assert call(nws=16) == -1                                   # workspace too small
    assert call(C=96) == -2                                     # three channel groups: the z-sliding kernel's
    assert call(both=ctypes.c_void_p(20)) == -4
    # host: a layer the op does not cover goes to conv3d_block (the z-sliding kernel) in run_block
    import torch.nn as nn
    from dsmnet_amd import blocks3d
    both = torch.zeros(2, 96, 5, 33, device="cuda").contiguous(memory_format=torch.channels_last)
    conv = nn.Conv3d(192, 32, 3, padding=1, bias=False).cuda()
    x = cv.VirtualVolume(both, 6, True)
    assert not cv.concat_conv_ok(x, 32)
    seen = []
    monkeypatch.setattr(cv, "conv3d_block", lambda *a, **k: seen.append(a[0]) or "zs")
    with torch.no_grad():
        assert blocks3d.run_block(blocks3d._Folded(), conv, None, x) == "zs" and seen == [x]


def test_run_block_switch_and_weight_cache(cv):
    """run_block takes the op when ``separable_volume`` is on, the z-sliding kernel when off; the packed
    weight follows in-place weight updates (tensor versions, as the other folded caches)."""
    import torch.nn as nn
    from dsmnet_amd import blocks3d
    shape, D = (1, 32, 6, 37), 9
    fL, fR = seeded(71, *shape), seeded(72, *shape)
    both = torch.cat([fL, fR], 0).cuda().contiguous(memory_format=torch.channels_last)
    conv = nn.Conv3d(64, 32, 3, padding=1, bias=False).cuda()
    folded = blocks3d._Folded()
    x = cv.VirtualVolume(both, D, True)
    names = []

    class Timer(cv.LaunchTimer):
        def stop(self, name, start, work):
            names.append(name)
    cv.set_timer(Timer())
    try:
        with torch.no_grad():
            with option(cv, "separable_volume", True):
                on = blocks3d.run_block(folded, conv, None, x, relu=blocks3d.RELU_AFTER_ADD)
            with option(cv, "separable_volume", False):
                off = blocks3d.run_block(folded, conv, None, x, relu=blocks3d.RELU_AFTER_ADD)
    finally:
        cv.set_timer(None)
    assert names[0] == "sepvol_fwd_kernel" and names[-1].startswith("conv3d_zs_") and names[-1].endswith("<vol>")
    assert maxerr(on, off) <= 2 * F16X2_MAX * off.abs().max().item()
    with torch.no_grad():
        conv.weight.mul_(2.0)
        with option(cv, "separable_volume", True):
            on2 = blocks3d.run_block(folded, conv, None, x, relu=blocks3d.RELU_AFTER_ADD)
    assert maxerr(on2, 2 * on) <= 1e-6 * on2.abs().max().item()


def _psmnet(golden_e2e):
    from tests.golden.make_goldens import images
    from tests.helpers import golden_state
    from dsmnet_amd.models import model_create_by_name
    sd, cfg = golden_state(golden_e2e, "psmnet")
    imL, imR = images(cfg["image_seed"], *cfg["hw"])
    m = model_create_by_name("psmnet", 192)
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval(), imL.cuda(), imR.cuda()


def test_psmnet_with_and_without_the_separable_volume(cv, golden_e2e):
    m, imL, imR = _psmnet(golden_e2e)
    outs = {}
    for on in (True, False):
        with option(cv, "separable_volume", on), torch.no_grad():
            outs[on] = m(imL, imR)[1]
        for pname, p in zip(("pred3", "pred2", "pred1"), outs[on]):
            golden_e2e.compare("e2e.psmnet." + pname, p, DISP_TOL)
    for a, b in zip(outs[True], outs[False]):
        print("separable on vs off: %.3g px" % maxerr(a, b))
        assert maxerr(a, b) <= DISP_TOL


def test_psmnet_graph_replay_is_bit_identical(cv, golden_e2e):
    from dsmnet_amd.graphs import GraphedForward
    m, imL, imR = _psmnet(golden_e2e)
    with option(cv, "separable_volume", True):
        g = GraphedForward(m, imL, imR)
        with torch.no_grad():
            want = [t.clone() for t in m(imL, imR)[1]]
        got = g(imL, imR)[1]
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        again = g(imL, imR)[1]
        for a, b in zip(again, want):
            assert torch.equal(a, b)


def test_gcnet_with_the_separable_volume(cv, golden_e2e):
    from tests.golden.make_goldens import images
    from tests.helpers import golden_state
    from dsmnet_amd.models import model_create_by_name
    sd, cfg = golden_state(golden_e2e, "gcnet")
    imL, imR = images(cfg["image_seed"], *cfg["hw"])
    m = model_create_by_name("gcnet", 192)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    names = []

    class Timer(cv.LaunchTimer):
        def stop(self, name, start, work):
            names.append(name)
    cv.set_timer(Timer())
    try:
        with option(cv, "separable_volume", True), torch.no_grad():
            _, (disp,) = m(imL.cuda(), imR.cuda())
    finally:
        cv.set_timer(None)
    assert "sepvol_fwd_kernel" in names
    golden_e2e.compare("e2e.gcnet.disp", disp, DISP_TOL)
